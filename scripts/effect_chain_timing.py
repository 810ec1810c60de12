#!/usr/bin/env python3
"""The effect chain on the device (Engine.effect_chain, k_chain_run / k_chain_map in csrc/chain.hip) on what the training
pre-processing augments: 24 and 128 float32 segments of 3 s, a program per segment drawn by simulate.draw_effects from
config/vctk_base_voicefixer_unet.json's probabilities and ranges where it sets them (treble, bass, high_pass, clip; low_pass and
reverse keep RandomServer's defaults), effect_list = treble, bass, low_pass, high_pass, clip, reverse.  In one process, the device
variants taking turns inside every repeat:

  a_chain_ms        ONE Engine.effect_chain call over all segments with the drawn programs (many are empty or short: the draw's)
  b_one_biquad_ms   ONE Engine.effect_chain call, every segment through one order-2 Butterworth low-pass of its own cut-off: a run
                    of one stage, one pass without padding
  c_four_biquads_ms ... through four biquads: still one pass, the cascade skewed over four lanes per segment
  d_all_six_ms      ... through treble, bass, low_pass, high_pass, clip, reverse: one cascade and one element-wise pass
  e_bank_ms         ONE Engine.sosfiltfilt_bank call over the same segments with the same order-2 Butterworth designs as (b): the
                    existing zero-phase filter, two passes over the padded segments, float64 out
  host_1t_s         simulate.chain_effects with the drawn programs on the host, one segment after the other, one thread

`*_ms` are HIP-event times around the Engine calls (the host work of a call -- cutting the programs into passes, the upload of the
pass table -- is inside when the device waits for it), `*_wall_ms` a host clock around the same calls up to a device synchronise;
after one warm-up call each, median of --reps.  Also whether (a) equals the host form bit for bit.  NOT measured: the list forms'
padding and download, the time per kernel (no profiler run), other segment lengths.  Run it under one time limit:

    timeout -k 10 600 python scripts/effect_chain_timing.py [--clips=24,128] [--seconds=3] [--reps=5] [--out=profiles/effect_chain_timing.json]
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
from voicefixer_main_amd import simulate  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
NAMES = ["treble", "bass", "low_pass", "high_pass", "clip", "reverse"]
P_EFFECTS = {
    "treble": {"prob": [0.05], "level": [3, 20]},
    "bass": {"prob": [0.15], "level": [3, 35]},
    "low_pass": {"prob": [0.3], "low_pass_range": [3000, 7000]},
    "high_pass": {"prob": [0.25], "high_pass_range": [500, 2000]},
    "clip": {"prob": [0.20], "louder_time": [1.0, 11.0]},
    "reverse": {"prob": [0.1]},
}


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


def workload(eng, n, L, reps):
    rng = np.random.default_rng(2026 + n)
    x = rng.uniform(-1, 1, (n, L)).astype(np.float32)
    xd = torch.from_numpy(x).to(eng.device)
    effects = simulate.draw_effects(n, P_EFFECTS, NAMES, 0, rng)
    drawn = [simulate._chain_steps(e) for e in effects]
    cuts = [float(rng.uniform(3000, 7000)) for _ in range(n)]
    one = [[("biquad", simulate.biquad_design("low_pass", f))] for f in cuts]
    shelf = [("biquad", simulate.biquad_design(name, v)) for name, v in (("treble", 6.0), ("bass", 12.0), ("high_pass", 800.0))]
    four = [p + shelf for p in one]
    six = [shelf[:2] + p + shelf[2:] + [("clip", 0.5), ("reverse",)] for p in one]
    bank = [signal.butter(2, f, fs=FS, output="sos") for f in cuts]
    variants = {
        "a_chain": lambda: eng.effect_chain(xd, drawn),
        "b_one_biquad": lambda: eng.effect_chain(xd, one),
        "c_four_biquads": lambda: eng.effect_chain(xd, four),
        "d_all_six": lambda: eng.effect_chain(xd, six),
        "e_bank": lambda: eng.sosfiltfilt_bank(xd, bank),
    }
    for fn in variants.values():      # warm-up: the scratch buffers, the tables, the code objects
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    steps = [len(p) for p in drawn]
    r = {"clips": n, "samples_per_clip": L, "drawn_steps_per_clip": {str(s): steps.count(s) for s in sorted(set(steps))},
         "drawn_biquads": sum(s[0] == "biquad" for p in drawn for s in p), "drawn_clips": sum(s[0] == "clip" for p in drawn for s in p),
         "drawn_reverses": sum(s[0] == "reverse" for p in drawn for s in p)}
    for k, v in ms.items():
        r[k + "_ms"] = round(float(np.median([e for e, _ in v])), 3)
        r[k + "_ms_all"] = [round(e, 3) for e, _ in v]
        r[k + "_wall_ms"] = round(float(np.median([w for _, w in v])), 3)
    r["b_over_e"] = round(r["b_one_biquad_ms"] / r["e_bank_ms"], 3)
    r["b_ns_per_step"] = round(r["b_one_biquad_ms"] * 1e6 / L, 1)
    t0 = time.perf_counter()
    host = [simulate.chain_effects(x[i], effects[i]) for i in range(n)]
    r["host_1t_s"] = round(time.perf_counter() - t0, 3)
    r["host_over_a"] = round(r["host_1t_s"] * 1e3 / r["a_chain_ms"], 2)
    r["bit_identical"] = bool(np.array_equal(variants["a_chain"]().cpu().numpy(), np.stack(host)))
    return r


def main():
    clips = opt("clips", [24, 128], lambda s: [int(v) for v in s.split(",")])
    seconds, reps = opt("seconds", 3.0), opt("reps", 5, int)
    out = opt("out", os.path.join(ROOT, "profiles", "effect_chain_timing.json"), str)
    torch.set_num_threads(1)
    eng = Engine("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": reps}
    for n in clips:
        res["clips_%d" % n] = workload(eng, n, int(seconds * FS), reps)
        print(json.dumps({n: res["clips_%d" % n]}), flush=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
