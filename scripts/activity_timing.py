#!/usr/bin/env python3
"""The record behind profiles/activity_timing.json: 128 float32 clips of 2-8 s (seeded, speech-like: bursts between silences), already
on the device as one padded batch -- the device time of Engine.trim_bounds (both grids), Engine.has_long_empty (3-s windows every
second) and Engine.active_frames between HIP events (median of --reps calls after two warm-up calls), the wall time of the host forms
of voicefixer_main_amd.activity on the same clips, and the time ONE read of the clips' samples takes at the HBM rate measured here
with a device-to-device copy of 1 GiB (read + write).

    python scripts/activity_timing.py [--clips=128] [--reps=8] [--out=profiles/activity_timing.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd import activity  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

THR = 500 / 2 ** 15


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


def make_clip(n, rng):
    x = np.zeros(n, np.float32)
    pos = int(rng.integers(0, 30000))
    while pos < n:
        burst, gap = int(rng.integers(4000, 60000)), int(rng.integers(2000, 50000))
        x[pos:pos + burst] = (0.2 * rng.standard_normal(burst)).astype(np.float32)[:max(0, n - pos)]
        pos += burst + gap
    return x


def main():
    n, reps = opt("clips", 128, int), opt("reps", 8, int)
    out = opt("out", os.path.join(ROOT, "profiles", "activity_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("activity_timing: no GPU")
    eng = Engine("cuda:0")
    rng = np.random.default_rng(2026)
    clips = [make_clip(int(rng.integers(2 * 44100, 8 * 44100 + 1)), rng) for _ in range(n)]
    lens = [len(c) for c in clips]
    x = torch.zeros((n, (max(lens) + 3) // 4 * 4), dtype=torch.float32)
    for b, c in enumerate(clips):
        x[b, :len(c)] = torch.from_numpy(c)
    x = x.to(eng.device)
    big = torch.empty(1 << 28, dtype=torch.float32, device=eng.device)
    copy_ms = timed(lambda: big.clone(), reps)
    rate = 2 * big.numel() * 4 / (copy_ms * 1e-3)
    del big
    rec = {"clips": n, "seconds": [2, 8], "samples": int(sum(lens)), "dtype": "float32", "threshold": THR,
           "trim_bounds_both_ms": timed(lambda: eng.trim_bounds(x, lens, THR), reps),
           "has_long_empty_ms": timed(lambda: eng.has_long_empty(x, lens, threshold=THR), reps),
           "active_frames_ms": timed(lambda: eng.active_frames(x, lens, THR), reps),
           "hbm_copy_rate_TBps": rate / 1e12, "one_read_of_the_batch_ms": sum(lens) * 4 / rate * 1e3}
    t = time.perf_counter()
    bounds = [activity.trim_bounds(c, THR) for c in clips]
    rec["host_trim_empty_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    flags = [activity.has_long_empty(c, threshold=THR) for c in clips]
    rec["host_has_long_empty_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    labels = [activity.get_all_active_segment_index(c, THR) for c in clips]
    rec["host_active_frames_ms"] = (time.perf_counter() - t) * 1e3
    s, e = eng.trim_bounds(x, lens, THR)
    assert [None if i < 0 else (i, j) for i, j in zip(s.cpu().tolist(), e.cpu().tolist())] == bounds
    assert [bool(f) for f in eng.has_long_empty(x, lens, threshold=THR).cpu().tolist()] == flags
    lab, cnt = eng.active_frames(x, lens, THR)
    lab = lab.cpu().numpy()
    assert all(lab[b, :c].tolist() == labels[b] for b, c in enumerate(cnt.cpu().tolist()))
    rec["kept_share"] = float(sum(b[1] - b[0] for b in bounds if b) / sum(lens))
    rec["long_empty"] = int(sum(flags))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
