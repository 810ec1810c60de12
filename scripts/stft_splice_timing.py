#!/usr/bin/env python3
"""The splice of a padded batch of clip pairs in one fused launch against the chain of launches it replaces, in one process:

  fused_ms         ONE Engine.stft_splice call on the padded batch between HIP events (the set-lengths launches, the fused launch and
                   the allocation of the output), after warm-up calls, median of --reps
  chain_ms         the same tree's unchanged launches on the same padded batch, timed the same way: torch multiply (g y) and
                   subtract, Engine.stft with phases (sp, cos, sin to memory), the torch products in the kernel's order (sp * cos and
                   sp * sin, each times the weights), Engine.istft, torch add.  The chain takes every row as a clip of the full width
                   -- it has no lengths -- so it transforms the padding too: chain_frames against fused_frames says how much more
  chain_over_fused their ratio
  sclk_mhz         the shader clock read from hwmon while the timed calls ran

for 128 float32 pairs of 2 .. 8 s, no two alike (the draw of bench.py's varlen workload: the launch with IH = 16), cut-off bin 372
(8 kHz), a ramp of 8 bins, a gain per clip.  Writes one JSON line to profiles/stft_splice_timing.json (or --out=).  Run it under one time
limit:

    timeout -k 10 600 python scripts/stft_splice_timing.py [--reps=7] [--out=profiles/stft_splice_timing.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import PowerSampler  # noqa: E402
from voicefixer_main_amd import clips as _clips, splice, synth  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
CUT, RAMP = 372, 8


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def event_ms(f, reps, device):
    for _ in range(3):      # warm-up: the code objects, the allocator's blocks
        f()
    torch.cuda.synchronize(device)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize(device)
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    reps = opt("reps", 7, int)
    out_path = opt("out", os.path.join(ROOT, "profiles", "stft_splice_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("stft_splice_timing: no GPU")
    eng = Engine("cuda:0")
    rng = np.random.default_rng(2025)      # bench.py, aux_varlen
    lens = sorted(int(v) for v in rng.uniform(2.0 * FS, 8.0 * FS, size=128))
    base = synth.make_clips(128, 8.1, seed=77)[:, 0]
    other = synth.make_clips(128, 8.1, seed=78)[:, 0]
    x = _clips.pad([base[i, :n] for i, n in enumerate(lens)], eng.device, torch.float32)
    y = _clips.pad([other[i, :n] for i, n in enumerate(lens)], eng.device, torch.float32)
    gains = [float(np.float32(v)) for v in rng.uniform(0.5, 2.0, size=128)]
    g = torch.tensor(gains, device=eng.device, dtype=torch.float32)[:, None]
    a = torch.from_numpy(splice.ramp_weights(CUT, RAMP)).to(eng.device)
    L = x.shape[1]

    def fused():
        return eng.stft_splice(x, y, CUT, lengths=lens, ramp=RAMP, gains=gains)

    def chain():
        gy = y * g
        o = eng.stft(x - gy, want_mel=False, want_sp=True, want_phase=True)
        return gy + eng.istft(o["sp"] * o["cos"] * a, o["sp"] * o["sin"] * a, L)

    with PowerSampler() as ps:
        res = {"clips": 128, "seconds": round(sum(lens) / FS, 2), "cut_bin": CUT, "ramp": RAMP, "reps": reps,
               "device": torch.cuda.get_device_name(0), "fused_frames": sum(n // eng.hop + 1 for n in lens),
               "chain_frames": 128 * (L // eng.hop + 1)}
        res["fused_ms"] = round(event_ms(fused, reps, eng.device), 3)
        res["chain_ms"] = round(event_ms(chain, reps, eng.device), 3)
    res["chain_over_fused"] = round(res["chain_ms"] / res["fused_ms"], 2)
    res["fused_audio_s_per_ms"] = round(res["seconds"] / res["fused_ms"], 1)
    # the longest clip fills its row: there the two must agree to the last bit
    res["longest_row_equal"] = bool(torch.equal(fused()[-1], chain()[-1]))
    power = ps.result() or {}
    res["sclk_mhz"], res["min_sclk_mhz"] = power.get("avg_sclk_mhz"), power.get("min_sclk_mhz")
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
