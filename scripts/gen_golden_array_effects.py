#!/usr/bin/env python3
"""Write tests/golden/array_effects.npz: the REFERENCE's own MagicalEffects.quantification and MagicalEffects.time_dropout
(dataloaders/augmentation/magical_effects.py:169-187, imported unmodified) on seeded float32 and float64 clips.

The packages the module imports at the top and these two functions never call (augment, librosa, git, ...) are stubbed with the two
stub sets of oracle/gen_golden.py.  Needs a checkout of the reference (--ref) and SciPy; runs on the CPU.  Never run by a test.

    python scripts/gen_golden_array_effects.py --ref <path to the reference checkout>

Keys: clip_<dtype>_<k> the clips; quant_<dtype>_<k>_b<bins> the quantiser's outputs; drop_params the (start, trunk_length) pairs and
drop_<dtype>_<k>_p<j> time_dropout's outputs (the function works in place: it is given a copy).
"""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (400, 997, 3000)
BINS = (1, 3, 8, 12)
# (start, trunk_length) as fractions of the clip.  For the shortest clip (400 samples): a plain stretch; patches that overlap (the
# stretch is shorter than a patch: 0, 10 and 60 samples); the first centre closer than 50 samples to the clip's start (skipped), the
# second one closer than 50 to its end (skipped), both; a stretch that runs past the end of the clip.
DROP_PARAMS = ((0.3, 0.2), (0.5, 0.0), (0.4, 0.025), (0.45, 0.15), (0.01, 0.3), (0.6, 0.39), (0.1, 0.85), (0.8, 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "array_effects.npz"))
    args = ap.parse_args()

    from oracle import gen_golden
    gen_golden.REF = os.path.abspath(args.ref)
    gen_golden.install_stubs()
    gen_golden.install_io_stubs()
    sys.path.insert(0, gen_golden.REF)
    from dataloaders.augmentation.magical_effects import MagicalEffects
    fx = MagicalEffects(p_effects=None)

    rng = np.random.default_rng(20201106)
    out = {"drop_params": np.asarray(DROP_PARAMS, dtype=np.float64), "bins": np.asarray(BINS), "lengths": np.asarray(LENGTHS)}
    for dtype in (np.float32, np.float64):
        name = np.dtype(dtype).name
        for k, n in enumerate(LENGTHS):
            clip = (rng.standard_normal(n) * rng.uniform(0.05, 0.9)).astype(dtype)
            out["clip_%s_%d" % (name, k)] = clip
            for bins in BINS:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    out["quant_%s_%d_b%d" % (name, k, bins)] = fx.quantification(clip.copy(), [True, bins])
            for j, (start, trunk) in enumerate(DROP_PARAMS):
                out["drop_%s_%d_p%d" % (name, k, j)] = fx.time_dropout(clip.copy(), [True, [start, trunk]])
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, "%d arrays, %d bytes" % (len(out), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
