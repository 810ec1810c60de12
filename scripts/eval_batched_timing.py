#!/usr/bin/env python3
"""A test set with targets through evaluation.inference (batched: VoiceFixer.restore_scored_list, the four mel scores computed on
the device inside vfx_restore_gsr_varlen_scored) against the way it was done before: handler_gsr_voicefixer once per file with its
target.  128 synthetic PCM16 pairs of 2-8 s (one fixed seed), synthetic weights, one process, wall time of a whole pass over the set
-- reading the files, restoring, scoring, writing the wav and JSON files -- up to a device synchronise; one warm-up pass of each, then
the median of --reps:

  inference_s / handler_s                  seconds per pass
  inference_audio_s_per_s / handler_...    audio seconds of the set per second of wall time
  ratio                                    inference's rate over the handler's
  score_max_abs_diff                       largest |inference's JSON - handler's dict| per key over the set

Writes one JSON document to profiles/eval_batched_timing.json (or --out=).  Run it under one time limit:

    timeout -k 10 900 python scripts/eval_batched_timing.py [--clips=128] [--reps=3] [--precision=2] [--out=...]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd import evaluation, handlers, metrics, synth  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402
from voicefixer_main_amd.models import HANDLER_METRIC_KEYS, VoiceFixer  # noqa: E402

FS = 44100


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def write_set(root, n_clips, seed=2027):
    """n_clips `noisy clean` pairs of 2-8 s under root/data, cut from eight synthetic voices -> (list path, audio seconds)"""
    rng = np.random.default_rng(seed)
    data = os.path.join(root, "data")
    os.makedirs(data)
    voices = [(synth.speech_like(8 * FS + 1, 4000 + v) * 0.6).astype(np.float32) for v in range(8)]
    lines, total = [], 0
    for i, n in enumerate(int(v) for v in rng.uniform(2 * FS, 8 * FS, size=n_clips)):
        clean = voices[i % 8][:n]
        noisy = synth.degrade(clean, 5000 + i, ("noise", "lowpass", "clip")[i % 3])
        src, tgt = os.path.join(data, "noisy%03d.wav" % i), os.path.join(data, "clean%03d.wav" % i)
        handlers.save_wave(noisy, src)
        handlers.save_wave(clean, tgt)
        lines.append("%s %s" % (src, tgt))
        total += n
    lst = os.path.join(root, "set.lst")
    with open(lst, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lst, lines, total / FS


def main():
    n_clips, reps, precision = opt("clips", 128, int), opt("reps", 3, int), opt("precision", 2, int)
    out_path = opt("out", os.path.join(ROOT, "profiles", "eval_batched_timing.json"), str)
    eng = Engine("cuda:0", config={"precision": precision})
    model = VoiceFixer(None, channels=2, type_target="vocals", engine=eng)
    sd = {"generator.analysis_module." + k: v for k, v in synth.make_resunet_state_dict(0).items()}
    sd.update({"vocoder.model." + k: v for k, v in synth.make_vocoder_state_dict(1).items()})
    model.load_state_dict(sd)
    model.eval()
    with tempfile.TemporaryDirectory() as root:
        lst, lines, seconds = write_set(root, n_clips)
        metas = {"set": {"rate": FS, "list": lst, "unify_energy": False}}
        by_handler = {}

        def batched(tag):
            evaluation.inference(model, os.path.join(root, "batched" + tag), ["set"], metas)

        def per_file(tag):
            res = os.path.join(root, "handler" + tag, "set")
            os.makedirs(res, exist_ok=True)
            for line in lines:
                src, tgt = line.split(" ")
                dst = os.path.join(res, os.path.basename(src))
                by_handler[os.path.basename(src)] = evaluation._run_handler(handlers.handler_gsr_voicefixer, model, src, dst, tgt, metas["set"])
                metrics.write_json(by_handler[os.path.basename(src)], dst[:-4] + ".json")

        times = {"inference": [], "handler": []}
        for r in range(reps + 1):                      # (pass 0 warms the plans, the scratch and the pinned buffers of both)
            for name, fn in (("inference", batched), ("handler", per_file)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(str(r))
                torch.cuda.synchronize()
                if r:
                    times[name].append(time.perf_counter() - t0)
        worst = dict.fromkeys(HANDLER_METRIC_KEYS, 0.0)
        for line in lines:
            name = os.path.basename(line.split(" ")[0])
            js = metrics.load_json(os.path.join(root, "batched%d" % reps, "set", name[:-4] + ".json"))
            for k in HANDLER_METRIC_KEYS:
                worst[k] = max(worst[k], abs(js[k] - by_handler[name][k]))
    t_inf, t_han = float(np.median(times["inference"])), float(np.median(times["handler"]))
    doc = {"clips": n_clips, "audio_s": seconds, "precision": precision, "reps": reps, "device": torch.cuda.get_device_name(0),
           "inference_s": t_inf, "handler_s": t_han, "inference_all_s": times["inference"], "handler_all_s": times["handler"],
           "inference_audio_s_per_s": seconds / t_inf, "handler_audio_s_per_s": seconds / t_han, "ratio": t_han / t_inf,
           "score_max_abs_diff": worst}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
