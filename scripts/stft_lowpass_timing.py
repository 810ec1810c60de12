#!/usr/bin/env python3
"""The "stft_hard" low-pass of a list of clips, as a batch and one clip per call, in one process:

  list_ms          simulate.lowpass_list(clips, 4000, 44100, _type="stft_hard", to_host=False), clips already on the device, wall
                   time with a device synchronisation, after warm-up calls, median of --reps.  On a tree whose Engine has
                   stft_lowpass this is the padded batches through the fused launch; on an older tree it is that tree's own loop
  per_clip_ms      the loop the list form replaced -- stft_hard_lowpass_v0 per clip (two launches, three torch element-wise
                   operations, one download) and the upload of its result -- timed the same way
  device_ms        ONE Engine.stft_lowpass call on the padded batch between HIP events (the set-lengths launches, the fused launch
                   and the allocation of the output), median of --reps; absent on an older tree
  sclk_mhz         the shader clock read from hwmon while the timed calls ran

for two sets: 128 float32 clips of 2 .. 8 s, no two alike (the draw of bench.py's varlen workload: the launch with IH = 16), and 4
clips of 3 s (IH = 2: every frame is transformed forward by three workgroups).  Writes one JSON line to
profiles/stft_lowpass_timing.json (or --out=).  Run it under one time limit:

    timeout -k 10 600 python scripts/stft_lowpass_timing.py [--reps=7] [--out=profiles/stft_lowpass_timing.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import PowerSampler  # noqa: E402
from voicefixer_main_amd import simulate, synth  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
HIGHCUT = 4000


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def wall_ms(f, reps, device):
    for _ in range(2):      # warm-up: the code objects, the allocator's blocks
        f()
    torch.cuda.synchronize(device)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize(device)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def measure(eng, clips, reps):
    ratio = HIGHCUT / int(FS / 2)
    res = {"clips": len(clips), "seconds": round(sum(c.shape[0] for c in clips) / FS, 2)}
    res["list_ms"] = round(wall_ms(lambda: simulate.lowpass_list(clips, HIGHCUT, FS, _type="stft_hard", engine=eng, to_host=False), reps,
                                   eng.device), 3)
    res["per_clip_ms"] = round(wall_ms(lambda: [torch.from_numpy(simulate.stft_hard_lowpass_v0(c.cpu().numpy(), ratio, engine=eng)).to(eng.device)
                                                for c in clips], reps, eng.device), 3)
    res["per_clip_over_list"] = round(res["per_clip_ms"] / res["list_ms"], 2)
    if hasattr(eng, "stft_lowpass"):
        from voicefixer_main_amd import clips as _clips
        order = sorted(range(len(clips)), key=lambda i: clips[i].shape[0])
        lens = [clips[i].shape[0] for i in order]
        x = _clips.pad([clips[i] for i in order], eng.device, torch.float32)
        cut = int(1025 * ratio)
        for _ in range(3):
            eng.stft_lowpass(x, cut, lengths=lens)
        torch.cuda.synchronize(eng.device)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.stft_lowpass(x, cut, lengths=lens)
            b.record()
            torch.cuda.synchronize(eng.device)
            ms.append(a.elapsed_time(b))
        res["device_ms"] = round(float(np.median(ms)), 3)
        res["device_audio_s_per_ms"] = round(res["seconds"] / res["device_ms"], 1)
    return res


def main():
    reps = opt("reps", 7, int)
    out_path = opt("out", os.path.join(ROOT, "profiles", "stft_lowpass_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("stft_lowpass_timing: no GPU")
    eng = Engine("cuda:0")
    rng = np.random.default_rng(2025)      # bench.py, aux_varlen
    lens = [int(v) for v in rng.uniform(2.0 * FS, 8.0 * FS, size=128)]
    base = synth.make_clips(128, 8.1, seed=77)[:, 0]
    varlen = [torch.from_numpy(base[i, :n].copy()).to(eng.device) for i, n in enumerate(lens)]
    four = [torch.from_numpy(base[i, :3 * FS].copy()).to(eng.device) for i in range(4)]
    with PowerSampler() as ps:
        res = {"highcut": HIGHCUT, "reps": reps, "device": torch.cuda.get_device_name(0), "fused": hasattr(eng, "stft_lowpass"),
               "varlen_128x2to8s": measure(eng, varlen, reps), "four_x_3s": measure(eng, four, reps)}
    power = ps.result() or {}
    res["sclk_mhz"], res["min_sclk_mhz"] = power.get("avg_sclk_mhz"), power.get("min_sclk_mhz")
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
