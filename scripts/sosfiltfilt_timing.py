#!/usr/bin/env python3
"""The device zero-phase IIR filter (Engine.sosfiltfilt, csrc/sosfilt.hip) on 128 float32 clips of 10 s, for the cheby1 order-8
low-pass at 1000 Hz and the cheby1 order-10 band-pass at 300-3400 Hz, in one process:

  device_ms        Engine.sosfiltfilt over the 128 clips as ONE call, HIP events, after a warm-up call, median of --reps
  device_b1_ms     the same for one clip
  scipy_1t_s       scipy.signal.sosfiltfilt over the same 128 clips on the host, one after the other
  scipy_pool_s     ... on a pool of --threads threads

and whether the batch result equals SciPy's bit for bit.  Run it under one time limit:

    timeout -k 10 600 python scripts/sosfiltfilt_timing.py [--clips=128] [--seconds=10] [--reps=5] [--threads=16] > profiles/sosfiltfilt_timing.json
"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def device_ms(eng, x, sos, reps):
    eng.sosfiltfilt(x, sos)                         # warm-up: the scratch buffer, the code object
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.sosfiltfilt(x, sos)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 3), [round(v, 3) for v in ms]


def main():
    n, seconds, reps, threads = opt("clips", 128, int), opt("seconds", 10.0), opt("reps", 5, int), opt("threads", 16, int)
    eng = Engine("cuda:0")
    L = int(seconds * FS)
    x = np.random.default_rng(2026).uniform(-1, 1, (n, L)).astype(np.float32)
    xd = torch.from_numpy(x).to(eng.device)
    res = {"clips": n, "samples_per_clip": L, "audio_seconds": round(n * L / FS, 1), "device": torch.cuda.get_device_name(0),
           "threads": threads}
    designs = {"cheby1_8_lowpass_1000": signal.cheby1(8, 0.1, 1000 / (FS / 2), btype="low", output="sos"),
               "cheby1_10_bandpass_300_3400": signal.cheby1(10, 0.1, [300 / (FS / 2), 3400 / (FS / 2)], btype="band", output="sos")}
    for name, sos in designs.items():
        r = {"sections": int(sos.shape[0])}
        r["device_ms"], r["device_ms_all"] = device_ms(eng, xd, sos, reps)
        r["device_b1_ms"], r["device_b1_ms_all"] = device_ms(eng, xd[:1], sos, reps)
        t0 = time.perf_counter()
        host = [signal.sosfiltfilt(sos, x[i]) for i in range(n)]
        r["scipy_1t_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda i: signal.sosfiltfilt(sos, x[i]), range(n)))
        r["scipy_pool_s"] = round(time.perf_counter() - t0, 3)
        r["pool_over_device"] = round(r["scipy_pool_s"] * 1e3 / r["device_ms"], 2)
        r["bit_identical"] = bool(np.array_equal(eng.sosfiltfilt(xd, sos).cpu().numpy(), np.stack(host)))
        res[name] = r
        print(json.dumps({name: r}), file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
