#!/usr/bin/env python3
"""The device RIR convolution (simulate.reverb_rir_list -> Engine.reverb_rir, csrc/reverb.hip) on a reverberant test set: 128 float32
clips of 2-8 s, each against its own synthetic RIR (synth.make_rir) of 0.3-1.0 s, in one process:

  device_ms        ONE reverb_rir_list(to_host=False) call over the set -- upload, padded batch, kernel, normalisation -- between HIP
                   events, after a warm-up call, median of --reps
  tflops           2 N M per clip over device_ms, and its fraction of the 157.3 TFLOP/s f32-matrix peak (an end-to-end rate: the
                   call includes the host-to-device copies)
  host_ms          scipy.signal.convolve over the same pairs on the host, one after the other (SciPy picks FFT at these sizes)
  sclk_mhz         the shader clock read from hwmon while the device calls ran

and the largest error of the device result against the float64 FFT convolution relative to the peak, for the record.  Writes one
JSON line to profiles/reverb_rir_timing.json (or --out=).  Run it under one time limit:

    timeout -k 10 600 python scripts/reverb_timing.py [--clips=128] [--reps=5] [--out=profiles/reverb_rir_timing.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import PowerSampler  # noqa: E402
from voicefixer_main_amd import simulate, synth  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
PEAK_TFLOPS = 157.3


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def main():
    n, reps = opt("clips", 128, int), opt("reps", 5, int)
    out_path = opt("out", os.path.join(ROOT, "profiles", "reverb_rir_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("reverb_timing: no GPU")
    eng = Engine("cuda:0")
    rng = np.random.default_rng(2026)
    clips = [(rng.uniform(-1, 1, int(s * FS)) * 0.3).astype(np.float32) for s in rng.uniform(2.0, 8.0, n)]
    rirs = [synth.make_rir(100 + i, int(s * FS)) for i, s in enumerate(rng.uniform(0.3, 1.0, n))]
    flop = float(sum(2.0 * c.shape[0] * r.shape[0] for c, r in zip(clips, rirs)))
    full_flop = float(sum(2.0 * (c.shape[0] + r.shape[0] - 1) * r.shape[0] for c, r in zip(clips, rirs)))

    simulate.reverb_rir_list(clips, rirs, engine=eng, to_host=False)      # warm-up: the code object, the allocator's blocks
    torch.cuda.synchronize()
    ms = []
    with PowerSampler() as ps:
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dev = simulate.reverb_rir_list(clips, rirs, engine=eng, to_host=False)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    power = ps.result() or {}
    device_ms = float(np.median(ms))

    t0 = time.perf_counter()
    host = [simulate.reverb_rir(c, r) for c, r in zip(clips, rirs)]
    host_ms = (time.perf_counter() - t0) * 1e3

    worst = 0.0
    for i in range(0, n, max(1, n // 8)):           # a sample of the set against the float64 convolution
        c, r = clips[i].astype(np.float64), rirs[i].astype(np.float64)
        want = simulate.reverb_rir(c, r)
        worst = max(worst, float(np.max(np.abs(dev[i].cpu().numpy() - want)) / np.max(np.abs(want))))
    res = {"clips": n, "audio_seconds": round(sum(c.shape[0] for c in clips) / FS, 1),
           "rir_seconds": round(sum(r.shape[0] for r in rirs) / FS, 1), "device": torch.cuda.get_device_name(0),
           "gflop_2NM": round(flop / 1e9, 1), "gflop_full_length": round(full_flop / 1e9, 1),
           "device_ms": round(device_ms, 3), "device_ms_all": [round(v, 3) for v in ms],
           "tflops": round(flop / device_ms / 1e9, 2), "fraction_of_f32_matrix_peak": round(flop / device_ms / 1e9 / PEAK_TFLOPS, 4),
           "host_ms": round(host_ms, 1), "host_over_device": round(host_ms / device_ms, 2),
           "sclk_mhz": power.get("avg_sclk_mhz"), "min_sclk_mhz": power.get("min_sclk_mhz"),
           "max_error_vs_float64_over_peak": worst,
           "host_equals_float32_fft_within": float(max(np.max(np.abs(host[i] - dev[i].cpu().numpy())) for i in range(0, n, max(1, n // 8))))}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
