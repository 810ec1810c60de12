#!/usr/bin/env python3
"""The device array effects (Engine.quantize, Engine.time_dropout, csrc/effects.hip) on 128 float32 clips of 3 s, in one process.  Per
effect:

  list_ms      ONE simulate.quantification_list / time_dropout_list call on the NumPy clips with to_host=False -- the padded batch
               built and uploaded, the launches -- between HIP events, after warm-up calls, median of --reps
  engine_ms    the Engine call alone on the batch already on the device (the output allocated, the launches), the same way
  host_ms      the loop over the host mirror on the same clips, one thread
  tb_per_s     the algorithmic traffic over engine_ms, and over list_ms: the quantiser reads every float32 sample twice (the peak
               pass, the map pass) and writes one float64, 16 B per sample; the drop-out reads it once and writes it once, 8 B

Writes one JSON line to profiles/array_effects_timing.json (or --out=).  Run it under one time limit:

    timeout -k 10 600 python scripts/array_effects_timing.py [--clips=128] [--seconds=3] [--reps=5] [--out=...]

Per kernel (profiles/array_effects_kernel_trace.txt), in a run of its own:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o NAME -- python scripts/array_effects_timing.py --out=DIR/timing.json
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd import clips as vclips, simulate  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
BYTES_PER_SAMPLE = {"quantize": 4 + 4 + 8, "time_dropout": 4 + 4}


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def timed(fn, reps):
    """median, min, max of `reps` calls between HIP events, after three warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    n, seconds, reps = opt("clips", 128, int), opt("seconds", 3.0), opt("reps", 5, int)
    out_path = opt("out", os.path.join(ROOT, "profiles", "array_effects_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("array_effects_timing: no GPU")
    torch.set_num_threads(1)
    eng = Engine("cuda:0")
    L = int(seconds * FS)
    rng = np.random.default_rng(2026)
    clips = [(rng.standard_normal(L) * rng.uniform(0.05, 0.5)).astype(np.float32) for _ in range(n)]
    bins = [int(b) for b in rng.integers(3, 12, n)]
    params = [[True, [float(rng.uniform(0.0, 0.8)), float(rng.uniform(0.0, 0.2))]] for _ in range(n)]
    ranges = [simulate._dropout_range(L, p) for p in params]
    x = vclips.pad(clips, eng.device, torch.float32, width=(L + 3) // 4 * 4)
    lens = [L] * n

    calls = {
        "quantize": (lambda: simulate.quantification_list(clips, bins, engine=eng, to_host=False),
                     lambda: eng.quantize(x, bins, lengths=lens),
                     lambda: [simulate.quantification(c, [True, b]) for c, b in zip(clips, bins)]),
        "time_dropout": (lambda: simulate.time_dropout_list(clips, params, engine=eng, to_host=False),
                         lambda: eng.time_dropout(x, [r[0] for r in ranges], [r[1] for r in ranges], lengths=lens),
                         lambda: [simulate.time_dropout(c.copy(), p) for c, p in zip(clips, params)]),
    }
    res = {"clips": n, "samples_per_clip": L, "dtype": "float32", "reps": reps, "device": torch.cuda.get_device_name(0)}
    for name, (list_fn, engine_fn, host_fn) in calls.items():
        list_ms, engine_ms = timed(list_fn, reps), timed(engine_fn, reps)
        t0 = time.perf_counter()
        want = host_fn()
        host_ms = (time.perf_counter() - t0) * 1e3
        got = list_fn()
        worst = max(float(np.max(np.abs(g.cpu().numpy().astype(np.float64) - w))) for g, w in zip(got[::16], want[::16]))
        gbytes = BYTES_PER_SAMPLE[name] * n * L / 1e9
        res[name] = {"list_ms": round(list_ms[0], 3), "list_ms_min": round(list_ms[1], 3), "list_ms_max": round(list_ms[2], 3),
                     "engine_ms": round(engine_ms[0], 3), "engine_ms_min": round(engine_ms[1], 3), "engine_ms_max": round(engine_ms[2], 3),
                     "host_ms": round(host_ms, 1), "host_over_list": round(host_ms / list_ms[0], 1),
                     "bytes_per_sample": BYTES_PER_SAMPLE[name], "gbytes": round(gbytes, 4),
                     "tb_per_s_engine": round(gbytes / engine_ms[0], 3), "tb_per_s_list": round(gbytes / list_ms[0], 4),
                     "max_abs_difference_from_host": worst}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
