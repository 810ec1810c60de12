#!/usr/bin/env python3
"""The zero-phase IIR filter with a design per clip (Engine.sosfiltfilt_bank, k_sosfilt_bank in csrc/sosfilt.hip) on what the
training collator filters: 24 and 128 float32 segments of 3 s, a low-pass per segment drawn by simulate.draw_lowpass_params from
config/vctk_base_voicefixer_unet.json's ranges (cut-off 750 .. 22 049 Hz, order 2 .. 10), IIR types only.  In one process, the
device variants taking turns inside every repeat:

  a_bank_ms            ONE Engine.sosfiltfilt_bank call over all segments
  b_per_design_ms      one Engine.sosfiltfilt call per distinct design over the segments that use it (gathered beforehand): what a
                       caller without the bank form has to do
  c_single_design_ms   ONE Engine.sosfiltfilt call over the same segments with a single order-10 design: the floor of a pass whose
                       time is set by the longest dependency chain, not by the number of clips
  scipy_1t_s           scipy.signal.sosfiltfilt with each segment's design on the host, one after the other
  scipy_pool_s         ... on a pool of --threads threads

`*_ms` are HIP-event times around the Engine calls (the host work of a call -- sosfilt_zi, the bank upload -- is inside when the
device waits for it), `*_wall_ms` a host clock around the same calls up to a device synchronise; after one warm-up call each, median
of --reps.  Also whether (a) equals SciPy bit for bit.  Run it under one time limit:

    timeout -k 10 600 python scripts/sosfilt_bank_timing.py [--clips=24,128] [--seconds=3] [--reps=5] [--threads=16] > profiles/sosfilt_bank_timing.json
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
from voicefixer_main_amd import simulate  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
IIR = ["cheby1", "ellip", "bessel", "butter"]


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def workload(eng, n, L, reps, threads):
    rng = np.random.default_rng(2026 + n)
    x = rng.uniform(-1, 1, (n, L)).astype(np.float32)
    xd = torch.from_numpy(x).to(eng.device)
    cutoffs, orders, types = simulate.draw_lowpass_params(n, [1500, 44100], [2, 10], IIR, rng)
    keys = sorted(set(zip(types, orders, cutoffs)))
    bank = [simulate._design(o, c / (0.5 * FS), "low", t, "lowpass") for t, o, c in keys]
    index = [keys.index(k) for k in zip(types, orders, cutoffs)]
    groups = [(bank[f], xd[[i for i in range(n) if index[i] == f]].contiguous()) for f in range(len(bank))]
    order10 = signal.cheby1(10, 0.1, 4000 / (0.5 * FS), output="sos")
    variants = {
        "a_bank": lambda: eng.sosfiltfilt_bank(xd, bank, filter_index=index),
        "b_per_design": lambda: [eng.sosfiltfilt(rows, sos) for sos, rows in groups],
        "c_single_design": lambda: eng.sosfiltfilt(xd, order10),
    }
    for fn in variants.values():      # warm-up: the scratch buffer, the bank buffer, the code objects
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    sections = [int(bank[f].shape[0]) for f in index]
    r = {"clips": n, "samples_per_clip": L, "distinct_designs": len(bank),
         "clips_per_section_count": {str(s): sections.count(s) for s in sorted(set(sections))}}
    for k, v in ms.items():
        r[k + "_ms"] = round(float(np.median([e for e, _ in v])), 3)
        r[k + "_ms_all"] = [round(e, 3) for e, _ in v]
        r[k + "_wall_ms"] = round(float(np.median([w for _, w in v])), 3)
    r["a_over_c"] = round(r["a_bank_ms"] / r["c_single_design_ms"], 2)
    r["b_over_a"] = round(r["b_per_design_ms"] / r["a_bank_ms"], 2)
    t0 = time.perf_counter()
    host = [signal.sosfiltfilt(bank[f], x[i]) for i, f in enumerate(index)]
    r["scipy_1t_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda i: signal.sosfiltfilt(bank[index[i]], x[i]), range(n)))
    r["scipy_pool_s"] = round(time.perf_counter() - t0, 3)
    r["pool_over_a"] = round(r["scipy_pool_s"] * 1e3 / r["a_bank_ms"], 2)
    r["bit_identical"] = bool(np.array_equal(variants["a_bank"]().cpu().numpy(), np.stack(host)))
    return r


def main():
    clips = opt("clips", [24, 128], lambda s: [int(v) for v in s.split(",")])
    seconds, reps, threads = opt("seconds", 3.0), opt("reps", 5, int), opt("threads", 16, int)
    eng = Engine("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "threads": threads, "reps": reps}
    for n in clips:
        res["clips_%d" % n] = workload(eng, n, int(seconds * FS), reps, threads)
        print(json.dumps({n: res["clips_%d" % n]}), file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
