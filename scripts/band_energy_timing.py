#!/usr/bin/env python3
"""The launches to put under `rocprofv3 --kernel-trace --stats` for profiles/band_energy_kernel_trace.txt: at 16 float32 clips of 10 s,
already on the device, --reps calls of Engine.band_energy (k_band_energy: ONE transform per frame at hop 512, k_band_cut) and --reps
calls of Engine.spec_losses on the same shape (k_pair_stft_l1: TWO transforms per frame at hop 441), after two warm-up calls of each.
Prints the median time of each call between HIP events.  Run it under one time limit:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d OUT -o band -- python scripts/band_energy_timing.py [--clips=16] [--reps=8]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd.engine import Engine  # noqa: E402


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def timed(call, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    n, seconds, reps = opt("clips", 16, int), opt("seconds", 10.0), opt("reps", 8, int)
    if not torch.cuda.is_available():
        raise SystemExit("band_energy_timing: no GPU")
    eng = Engine("cuda:0")
    rng = np.random.default_rng(2026)
    x = torch.from_numpy((0.05 * rng.standard_normal((n, int(seconds * 44100)))).astype(np.float32)).to(eng.device)
    y = torch.from_numpy((0.05 * rng.standard_normal(tuple(x.shape))).astype(np.float32)).to(eng.device)
    print("clips=%d samples=%d band_energy_ms=%.3f spec_losses_ms=%.3f" % (n, x.shape[1], timed(lambda: eng.band_energy(x), reps),
                                                                           timed(lambda: eng.spec_losses(x, y), reps)))


if __name__ == "__main__":
    main()
