#!/usr/bin/env python3
"""Scoring a restored test set (AudioMetrics / aggregate_score, voicefixer_main_amd/metrics.py) on the 128 clips of 2-8 s of the
varlen workload (scripts/bench_varlen.py: the same lengths), timed four ways:

  device_ms        vfx_audio_metrics over the 128 pairs as ONE call (sorted by length), HIP events, median of --reps
  stoi_device_ms   with --stoi: vfx_stoi over the same 128 pairs as one call, timed the same way (report only)
  bsseval_device_ms  with --bsseval: vfx_bsseval (512 taps) over the same 128 pairs as one call, timed the same way (report only), its
                   share of restore_list_s, and the float64 numpy restatement (tests/bsseval_f64.py) on --threads threads
  restore_list_s   VoiceFixer.restore_list on the same clips (synthetic weights, --precision), wall, median: the bar is
                   device_ms <= 10 % of it
  aggregate_s      aggregate_score end to end: 128 PCM16 est files and 128 targets read, scored, JSON / CSV / result.json written
  numpy_s          the float64 numpy restatement (tests/audio_metrics_f64.py) over the same pairs on --threads threads

    python scripts/bench_scoring.py [--clips=128] [--reps=5] [--precision=2] [--threads=16] [--only-device] [--stoi] [--bsseval] > scoring.json
"""
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd import handlers, metrics, models, synth  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def pcm(x):
    return ((np.asarray(x, np.float64) * 2 ** 15).astype(np.short) / 32768.0).astype(np.float32)


def main():
    n, reps, precision, threads = opt("clips", 128, int), opt("reps", 5, int), opt("precision", 2, int), opt("threads", 16, int)
    dev = torch.device("cuda:0")
    eng = Engine(dev, config={"precision": precision})
    rng = np.random.default_rng(2025)
    lens = [int(v) for v in rng.uniform(2 * 44100, 8 * 44100, size=n)]      # bench_varlen.py's clips
    est_all = synth.make_clips(n, 8.1, seed=77)[:, 0]
    tgt_all = synth.make_clips(n, 8.1, seed=78)[:, 0]
    ests = [pcm(est_all[i, :L]) for i, L in enumerate(lens)]
    tgts = [pcm(0.7 * est_all[i, :L] + 0.3 * tgt_all[i, :L]) for i, L in enumerate(lens)]
    total = sum(lens) / 44100.0
    res = {"clips": n, "audio_seconds": round(total, 1)}

    order = sorted(range(n), key=lambda i: lens[i])
    Lmax = max(lens)
    e = torch.zeros(n, Lmax)
    t = torch.zeros(n, Lmax)
    for j, i in enumerate(order):
        e[j, :lens[i]] = torch.from_numpy(ests[i])
        t[j, :lens[i]] = torch.from_numpy(tgts[i])
    e, t = e.to(dev), t.to(dev)
    ls = [lens[i] for i in order]

    def device_ms(call):
        call()                                      # workspace
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    ms = device_ms(lambda: eng.audio_metrics(e, t, ls))
    res["device_ms"] = round(float(np.median(ms)), 3)
    res["device_ms_all"] = [round(v, 3) for v in ms]
    res["device_audio_s_per_s"] = round(total / (res["device_ms"] / 1e3), 1)
    if "--stoi" in sys.argv:
        ms = device_ms(lambda: eng.stoi(e, t, ls, fs=44100))
        res["stoi_device_ms"] = round(float(np.median(ms)), 3)
        res["stoi_device_ms_all"] = [round(v, 3) for v in ms]
    if "--bsseval" in sys.argv:
        ms = device_ms(lambda: eng.bsseval(e, t, ls))
        res["bsseval_device_ms"] = round(float(np.median(ms)), 3)
        res["bsseval_device_ms_all"] = [round(v, 3) for v in ms]
    if "--only-device" in sys.argv:                 # (a profiler run: nothing but the scoring call in the trace)
        print(json.dumps(res))
        return

    m = models.VoiceFixer(None, channels=2, type_target="vocals", engine=eng)
    sd = {"generator.analysis_module." + k: v for k, v in synth.make_resunet_state_dict(0).items()}
    sd.update({"vocoder." + k: v for k, v in synth.make_vocoder_state_dict(1).items()})
    m.load_state_dict(sd)
    clips = [torch.from_numpy(x).to(dev) for x in ests]
    m.restore_list(clips)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.restore_list(clips)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    res["restore_list_s"] = round(float(np.median(ts)), 4)
    res["device_over_restore_list"] = round(res["device_ms"] / 1e3 / res["restore_list_s"], 4)
    if "--bsseval" in sys.argv:
        res["bsseval_over_restore_list"] = round(res["bsseval_device_ms"] / 1e3 / res["restore_list_s"], 4)
    print(json.dumps(res), flush=True)

    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "out", "bench"))
        lines = []
        for i in range(n):
            src, tgt = os.path.join(d, "n%03d.wav" % i), os.path.join(d, "c%03d.wav" % i)
            handlers.save_wave(tgts[i], tgt)
            handlers.save_wave(ests[i], os.path.join(d, "out", "bench", "n%03d.wav" % i))
            lines.append("%s %s" % (src, tgt))
        with open(os.path.join(d, "bench.lst"), "w") as f:
            f.write("\n".join(lines) + "\n")
        metas = {"bench": {"rate": 44100, "list": os.path.join(d, "bench.lst")}}
        ts = []
        for _ in range(max(1, reps // 2)):
            t0 = time.perf_counter()
            out = metrics.aggregate_score(os.path.join(d, "out"), ["bench"], metas=metas, engine=eng)
            ts.append(time.perf_counter() - t0)
        assert len(out["bench"]) == n
        res["aggregate_s"] = round(float(np.median(ts)), 3)
        res["aggregate_audio_s_per_s"] = round(total / res["aggregate_s"], 1)
    print(json.dumps(res), flush=True)

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import audio_metrics_f64 as ref
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        host = list(ex.map(lambda i: ref.audio_metrics(ests[i], tgts[i]), range(n)))
    res["numpy_threads"] = threads
    res["numpy_s"] = round(time.perf_counter() - t0, 2)
    res["numpy_audio_s_per_s"] = round(total / res["numpy_s"], 1)
    got = eng.audio_metrics(e, t, ls).cpu().numpy()
    want = np.stack([host[i] for i in order])
    res["max_abs_diff_vs_numpy"] = [float(v) for v in np.abs(got - want).max(axis=0)]
    if "--bsseval" in sys.argv:
        import bsseval_f64 as bref
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            host = list(ex.map(lambda i: bref.bsseval(ests[i], tgts[i]), range(n)))
        res["bsseval_numpy_s"] = round(time.perf_counter() - t0, 2)
        got = eng.bsseval(e, t, ls).cpu().numpy()
        res["bsseval_max_abs_diff_vs_numpy"] = [float(v) for v in np.abs(got - np.stack([host[i] for i in order])).max(axis=0)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
