#!/usr/bin/env python3
"""Times of the three analysis modules of Generator (mel ResUNet, bi_gru, dnn): vfx_restore_gsr at 16 x 10 s and 1 x 60 s with
each module selected, and the module alone (vfx_analysis_mel / vfx_resunet_mel) on the same mel shapes.  Median of --steps
timed calls after --warmup, HIP events on the current stream; one JSON line per (module, shape, stage).

    python scripts/bench_analysis.py --precision 1 --steps 20 --warmup 3 [--out profiles/analysis_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd import synth  # noqa: E402
from voicefixer_main_amd.engine import Engine, MODEL_DNN_MEL, MODEL_GRU_MEL, MODEL_UNET_MEL, MODEL_VOCODER  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modules", default="unet,bi_gru,dnn")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = Engine("cuda:0", config={"precision": args.precision})
    eng.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
    eng.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
    eng.load_state_dict(MODEL_GRU_MEL, synth.make_gru_analysis_state_dict())
    eng.load_state_dict(MODEL_DNN_MEL, synth.make_dnn_analysis_state_dict())
    ids = {"unet": MODEL_UNET_MEL, "bi_gru": MODEL_GRU_MEL, "dnn": MODEL_DNN_MEL}
    rows = []
    for B, sec in ((16, 10.0), (1, 60.0)):
        wav = torch.from_numpy(synth.make_clips(B, sec, seed=7)[:, 0]).cuda()
        mel = eng.stft(wav)["mel"]
        T = mel.shape[1]
        for name in args.modules.split(","):
            mid = ids[name]
            eng.select_analysis(mid)
            out = torch.empty_like(wav)
            med, lo, hi = timed(lambda: eng.restore_gsr(wav, out=out), args.steps, args.warmup)
            rows.append(dict(module=name, B=B, seconds=sec, T=T, stage="restore_gsr", ms_median=med, ms_min=lo, ms_max=hi,
                             audio_s_per_s=B * sec / (med / 1e3)))
            med, lo, hi = timed(lambda: eng.analysis_mel(mid, mel), args.steps, args.warmup)
            rows.append(dict(module=name, B=B, seconds=sec, T=T, stage="analysis", ms_median=med, ms_min=lo, ms_max=hi))
            assert eng.take_flags() == 0
    eng.select_analysis(MODEL_UNET_MEL)
    for r in rows:
        r["precision"] = args.precision
        print(json.dumps(r))
    if args.out:
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
