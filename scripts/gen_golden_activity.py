#!/usr/bin/env python3
"""Write tests/golden/activity.npz: the REFERENCE's own peak-threshold silence functions (tools/others/audio_op.py:71-150, imported
unmodified) on a few seeded clips -- trim_tail_empty, trim_head_empty, trim_empty, has_long_empty, get_all_active_segment_index,
is_valid_signal and max_mag_unify.

The file holds inputs, thresholds, bounds, flags and labels only.  The module's imports that do not exist offline are stubbed in
sys.modules before it is imported: `tools.file.wav` (a star import that brings np and os) and `librosa`, of which the module uses
librosa.util.pad_center alone: np.pad with (size - n) // 2 samples on the left and the rest on the right, librosa's definition.
The functions return views of their input; a view's bounds are read off its length: the tail keeps [0, len), the head [n - len, n).
The clips are on the PCM scale the reference's defaults (500, 400) are meant for, integer-valued so that the file stays small.
Needs a checkout of the reference (--ref) and NumPy >= 2 (a Python threshold against a float32 clip is compared in float32).

    python scripts/gen_golden_activity.py --ref <path to the reference checkout>
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (threshold, sample_rate, frame_length) of the trims; (threshold, sample_rate, frame_length, frame_shift) of the labels;
# (length, sample_rate) of has_long_empty, whose threshold is the reference's 400
TRIMS = ((500, 44100, 0.02), (150.5, 44100, 0.02), (500, 8000, 0.016))
FRAMES = ((500, 44100, 0.02, 0.01), (1000, 16000, 0.02, 0.01))
LONGS = ((3, 300), (1, 1000))
LENGTHS = (0, 500, 881, 882, 883, 1764, 2065, 3528, 4511, 6003, 9001)


def import_reference(ref):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def pad_center(data, size, axis=-1, **kwargs):
        n = data.shape[axis]
        lpad = int((size - n) // 2)
        lengths = [(0, 0)] * data.ndim
        lengths[axis] = (lpad, int(size - n - lpad))
        return np.pad(data, lengths, **kwargs)

    for name in ("tools", "tools.file"):
        stub(name)
    stub("tools.file.wav", np=np, os=os)
    stub("librosa", util=stub("librosa.util", pad_center=pad_center))
    spec = importlib.util.spec_from_file_location("ref_audio_op", os.path.join(ref, "tools", "others", "audio_op.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_clip(n, seed, dtype):
    """Bursts of integer-valued "speech" (peaks up to 3000) between stretches of silence and of a hum below every threshold used"""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=dtype)
    pos = int(rng.integers(0, max(1, min(1500, n // 2))))
    while pos < n:
        burst = int(rng.integers(40, 900))
        x[pos:pos + burst] = rng.integers(-3000, 3001, size=min(burst, n - pos))
        gap = int(rng.integers(300, 2600))
        if rng.random() < 0.5:
            x[pos + burst:pos + burst + gap] = rng.integers(-140, 141, size=max(0, min(gap, n - pos - burst)))
        pos += burst + gap
    return x


def bounds_of(ref, x, threshold, sample_rate, frame_length):
    """(3, 2) int64: what tail, head and both keep of x, -1 / -1 for None"""
    n = x.shape[0]
    kw = dict(threshold=threshold, sample_rate=sample_rate, frame_length=frame_length)
    out = np.full((3, 2), -1, dtype=np.int64)
    t = ref.trim_tail_empty(x, **kw)
    if t is not None:
        out[0] = (0, t.shape[0])
    h = ref.trim_head_empty(x, **kw)
    if h is not None:
        out[1] = (n - h.shape[0], n)
    e = ref.trim_empty(x, **kw)
    if e is not None:
        out[2] = (t.shape[0] - e.shape[0], t.shape[0])
        assert np.array_equal(e, x[out[2, 0]:out[2, 1]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "activity.npz"))
    args = ap.parse_args()
    assert int(np.__version__.split(".")[0]) >= 2, "NumPy >= 2: the comparisons of a float32 clip with a Python scalar"
    ref = import_reference(args.ref)
    out = {"trims": np.array(TRIMS, dtype=np.float64), "frames": np.array(FRAMES, dtype=np.float64),
           "longs": np.array(LONGS, dtype=np.float64), "lengths": np.array(LENGTHS, dtype=np.int64)}
    for i, n in enumerate(LENGTHS):
        x = make_clip(n, 100 + i, np.float64 if i % 3 == 2 else np.float32)
        if n == 3528:
            x[:] = 0  # all silent
            x[7] = 120
        if n == 1764:
            x[:] = 0  # active only in its last 20-ms segment: the tail keeps it whole, the head finds nothing before n - seg
            x[900:1300] = 2000
        out["x%d" % i] = x
        out["bounds%d" % i] = np.stack([bounds_of(ref, x, *p) for p in TRIMS])
        out["long%d" % i] = np.array([ref.has_long_empty(x, length=l, sample_rate=sr) for l, sr in LONGS], dtype=np.int64)
        for j, (thr, sr, fl, fs) in enumerate(FRAMES):
            if n > int(fs * sr):  # (np.pad's reflect mode wants a sample to reflect)
                out["labels%d_%d" % (i, j)] = np.array(ref.get_all_active_segment_index(x, thr, sr, fl, fs), dtype=np.uint8)
        if n:
            out["valid%d" % i] = np.array([ref.is_valid_signal(x, threshold=t) for t in (1000, 2999, 3000)], dtype=np.int64)
    pairs = ((5, 4), (9, 7), (8, 2))  # (ref, est): float64 / float32, float32 / float32, float64 / float64
    out["unify_pairs"] = np.array(pairs, dtype=np.int64)
    for j, (a, b) in enumerate(pairs):
        r, e = ref.max_mag_unify(out["x%d" % a], out["x%d" % b])
        assert r is out["x%d" % a]
        out["unify%d" % j] = e
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
