#!/usr/bin/env python3
"""The device noise mixer (Engine.mix_noise, csrc/mix.hip) on a training-sized batch: 128 float32 clips of 10 s, the form with HQ and
Aug and the noisy output, every tensor already on the device, in one process:

  device_ms        ONE Engine.mix_noise call -- the memset and the five launches of csrc/mix.hip, and the allocation of the five
                   output tensors -- between HIP events, after warm-up calls, median of --reps
  bytes_per_sample what the passes must move per clip-sample: 4 B x (4 reads for the peaks + 2 for the level sums + 2 for the
                   mixture's peak + 4 reads and 5 writes for the apply pass) = 68 B
  tb_per_s         bytes_per_sample x samples over device_ms, and its fraction of the 8.0 TB/s HBM peak (6.3 TB/s is what a
                   float4 copy reaches on this part)
  host_ms          the loop over simulate.add_noise_and_scale_with_HQ_with_Aug on the same clips, with the same draws
  sclk_mhz         the shader clock read from hwmon while the device calls ran

and the largest relative error of a sample of the device clips against the host function in float64.  Writes one JSON line to
profiles/mix_noise_timing.json (or --out=).  Run it under one time limit:

    timeout -k 10 600 python scripts/mix_noise_timing.py [--clips=128] [--seconds=10] [--reps=20] [--out=profiles/mix_noise_timing.json]
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
from voicefixer_main_amd import simulate  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
PEAK_TBS = 8.0
BYTES_PER_SAMPLE = 4 * (4 + 2 + 2 + 4 + 5)


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def main():
    n, seconds, reps = opt("clips", 128, int), opt("seconds", 10.0), opt("reps", 20, int)
    out_path = opt("out", os.path.join(ROOT, "profiles", "mix_noise_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("mix_noise_timing: no GPU")
    eng = Engine("cuda:0")
    L = int(seconds * FS)
    rng = np.random.default_rng(2026)
    names = ("hq", "front", "aug", "noise")
    host = {k: (rng.standard_normal((n, L)) * rng.uniform(0.05, 0.5, (n, 1))).astype(np.float32) for k in names}
    dev = {k: torch.from_numpy(v).to(eng.device) for k, v in host.items()}
    snr, scale = rng.uniform(-5, 35, n), rng.uniform(0.6, 1.0, n)
    kw = dict(noise_weight=[10 ** (s / 20) for s in snr], scale=list(scale), want_noisy=True)

    for _ in range(3):      # warm-up: the code object, the scratch buffer, the allocator's blocks
        y = eng.mix_noise(**dev, **kw)
    torch.cuda.synchronize()
    ms = []
    with PowerSampler() as ps:
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            y = eng.mix_noise(**dev, **kw)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    power = ps.result() or {}
    device_ms = float(np.median(ms))

    class Draws:      # the host loop with the device call's draws: snr then scale per clip
        def __init__(self, values):
            self.values = iter(values)

        def random(self):
            return next(self.values)
    unit = Draws([v for i in range(n) for v in ((snr[i] + 5) / 40, (scale[i] - 0.6) / 0.4)])
    t0 = time.perf_counter()
    ref = [simulate.add_noise_and_scale_with_HQ_with_Aug(*[host[k][i] for k in names], rng=unit) for i in range(n)]
    host_ms = (time.perf_counter() - t0) * 1e3

    worst = 0.0
    for i in range(0, n, max(1, n // 8)):      # a sample of the batch against the host function in float64, at the device's draws
        want = simulate.add_noise_and_scale_with_HQ_with_Aug(*[host[k][i].astype(np.float64) for k in names], snr_l=snr[i], snr_h=snr[i],
                                                             scale_lower=scale[i], scale_upper=scale[i])
        for k, w in zip(names, want):
            worst = max(worst, float(np.max(np.abs(y[k][i].cpu().numpy() - w) / np.abs(w))))
    samples = n * L
    tbs = BYTES_PER_SAMPLE * samples / device_ms / 1e9
    res = {"clips": n, "samples_per_clip": L, "form": 2, "want_noisy": True, "device": torch.cuda.get_device_name(0),
           "device_ms": round(device_ms, 3), "device_ms_min": round(min(ms), 3), "device_ms_max": round(max(ms), 3), "reps": reps,
           "bytes_per_sample": BYTES_PER_SAMPLE, "gbytes": round(BYTES_PER_SAMPLE * samples / 1e9, 3), "tb_per_s": round(tbs, 3),
           "fraction_of_hbm_peak": round(tbs / PEAK_TBS, 4), "host_ms": round(host_ms, 1),
           "host_over_device": round(host_ms / device_ms, 1), "sclk_mhz": power.get("avg_sclk_mhz"),
           "min_sclk_mhz": power.get("min_sclk_mhz"), "max_rel_error_vs_float64_x_2p24": round(worst * 2 ** 24, 2),
           "host_f32_first_noise_sample": float(ref[0][3][0]), "device_first_noise_sample": float(y["noise"][0, 0])}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
