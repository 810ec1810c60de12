#!/usr/bin/env python3
"""The training collator's low-pass with the "stft" follow-ups on the device (Engine.resample_each, k_resample_each in
csrc/resample.hip): simulate.lowpass_collate over 16 items of 3 s with a `vocals` and a `noise` key, all six filter types,
low_pass_range = (2000, 44100), orders 2 .. 10, one fixed seed -- every call draws the same cut-offs.  In one process, wall time up to
a device synchronise, one warm-up call and the median of --reps each:

  collate_warm_ms      this tree, the taps cache warm (every design of the batch already on the device)
  collate_cold_ms      this tree, the taps cache emptied before every call: SciPy's firwin runs on the host for every distinct M;
                       firwin_ms is the part of that call spent inside firwin, firwin_share its share
  collate_parent_ms    --parent-simulate=FILE: the simulate.py of the parent commit (its "stft" items go to the host unless
                       Engine.resample takes the pair, float32 only) on this tree's engine and the same inputs and draws;
                       parent_equal: its tensors equal this tree's bit for bit
  stft_scipy_1t_ms     the bare "stft" pass of the batch -- stft_hard_lowpass on every item that takes it, on the rows the collator
                       hands it -- through SciPy on one thread, and
  stft_scipy_pool_ms   on a pool of --threads threads
  each_down_ms / each_up_ms    ONE Engine.resample_each call each (down, then up with n_out) over those rows as one float64 batch
                       between HIP events, taps cache warm: the cat of the designs, the scaling launch and k_resample_each;
  each_down_natural_ms / each_up_natural_ms    the same with the handle's debug switch on: the scaled taps in natural order
  sclk_mhz             the shader clock read from hwmon while the calls ran

--launches=N runs nothing but N warm down / up call pairs (--natural=1: natural tap order), for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o NAME -- python scripts/resample_each_timing.py --launches=5

Writes one JSON document to profiles/resample_each_timing.json (or --out=).  Run it under one time limit:

    timeout -k 10 600 python scripts/resample_each_timing.py [--reps=5] [--threads=16] [--parent-simulate=FILE] [--out=...]
"""
import importlib.util
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import PowerSampler  # noqa: E402
from voicefixer_main_amd import _lib, simulate  # noqa: E402
from voicefixer_main_amd import clips as _clips  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
TYPES = ["butter", "cheby1", "ellip", "bessel", "stft", "stft_hard"]
RANGE, ORDERS, SEED = (2000, 44100), (2, 10), 2026


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def wall_ms(f, reps, before=None):
    """one warm-up call, then the median of `reps` (and every time); `before` runs outside the clock"""
    ts = []
    for i in range(reps + 1):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts[1:])), 3), [round(t, 3) for t in ts[1:]]


def event_ms(f, reps):
    f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 3)


def load_parent(path):
    spec = importlib.util.spec_from_file_location("voicefixer_main_amd._parent_simulate", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def stft_rows(eng, batch):
    """The rows and cut-offs of every "stft" pass lowpass_collate runs on this batch with the seed's draws: recorded from a run."""
    rows = []
    inner = simulate._stft_list

    def recording(clips, ratios, engine, to_host, fs_ori=44100):
        rows.extend((_clips.as_numpy(c).copy(), r) for c, r in zip(clips, ratios))
        return inner(clips, ratios, engine, to_host, fs_ori)

    simulate._stft_list = recording
    try:
        collate(simulate, eng, batch)
    finally:
        simulate._stft_list = inner
    return rows


def collate(sim, eng, batch):
    return sim.lowpass_collate(batch, RANGE, ORDERS, TYPES, FS, rng=np.random.default_rng(SEED), engine=eng)


def main():
    reps, threads = opt("reps", 5, int), opt("threads", 16, int)
    items, seconds = opt("items", 16, int), opt("seconds", 3.0)
    launches, natural = opt("launches", 0, int), opt("natural", 0, int)
    parent_path = opt("parent-simulate", "", str)
    out_path = opt("out", os.path.join(ROOT, "profiles", "resample_each_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("resample_each_timing: no GPU")
    eng = Engine("cuda:0")
    tlib = _lib.load_test()
    L = int(seconds * FS)
    data = np.random.default_rng(SEED + 1)
    batch = [{"fname": "item%d" % i, "vocals": data.uniform(-1, 1, (L, 1)).astype(np.float32),
              "noise": data.uniform(-1, 1, (L, 1)).astype(np.float32)} for i in range(items)]
    rows = stft_rows(eng, batch)
    downs = [int(r * FS) for _, r in rows]
    x64 = _clips.pad([c for c, _ in rows], eng.device, torch.float64)

    def down_up(which=None):
        low, lens = eng.resample_each(x64, FS, downs)
        if which == "down":
            return low, lens
        return eng.resample_each(low, downs, FS, lengths=lens, n_out=L)

    if launches:
        tlib.vfx_debug_resample_each_layout(eng.h, natural)
        for _ in range(launches + 1):
            down_up()
        torch.cuda.synchronize()
        return

    res = {"device": torch.cuda.get_device_name(0), "items": items, "samples_per_item": L, "reps": reps, "threads": threads,
           "stft_rows": len(rows), "stft_rows_float64": sum(1 for c, _ in rows if c.dtype == np.float64),
           "distinct_M": len({max(Engine.resample_ratio(FS, d)) for d in downs}),
           "taps_total": int(sum(20 * m + 1 for m in {max(Engine.resample_ratio(FS, d)) for d in downs}))}
    with PowerSampler() as ps:
        res["collate_warm_ms"], res["collate_warm_ms_all"] = wall_ms(lambda: collate(simulate, eng, batch), reps)
        import scipy.signal
        firwin, spent = scipy.signal.firwin, [0.0]

        def timed_firwin(*a, **kw):
            t0 = time.perf_counter()
            try:
                return firwin(*a, **kw)
            finally:
                spent[0] += (time.perf_counter() - t0) * 1e3

        scipy.signal.firwin = timed_firwin
        try:
            res["collate_cold_ms"], res["collate_cold_ms_all"] = wall_ms(lambda: collate(simulate, eng, batch), reps,
                                                                         before=eng._resample_each_cache.clear)
        finally:
            scipy.signal.firwin = firwin
        res["firwin_ms"] = round(spent[0] / (reps + 1), 3)
        res["firwin_share"] = round(res["firwin_ms"] / res["collate_cold_ms"], 3)
        if parent_path:
            parent = load_parent(parent_path)
            res["collate_parent_ms"], res["collate_parent_ms_all"] = wall_ms(lambda: collate(parent, eng, batch), reps)
            a, b = collate(simulate, eng, batch), collate(parent, eng, batch)
            res["parent_equal"] = all(torch.equal(a[k], b[k]) for k in a if k != "fname")
            res["parent_over_warm"] = round(res["collate_parent_ms"] / res["collate_warm_ms"], 2)
            res["parent_over_cold"] = round(res["collate_parent_ms"] / res["collate_cold_ms"], 2)
        low, lens = down_up("down")
        for layout, name in ((0, ""), (1, "_natural")):
            tlib.vfx_debug_resample_each_layout(eng.h, layout)
            res["each_down%s_ms" % name] = event_ms(lambda: down_up("down"), reps)
            res["each_up%s_ms" % name] = event_ms(lambda: eng.resample_each(low, downs, FS, lengths=lens, n_out=L), reps)
        tlib.vfx_debug_resample_each_layout(eng.h, 0)
    power = ps.result() or {}
    res["sclk_mhz"], res["min_sclk_mhz"] = power.get("avg_sclk_mhz"), power.get("min_sclk_mhz")

    def host(i):
        return simulate.stft_hard_lowpass(rows[i][0], rows[i][1])

    def serial():
        return [host(i) for i in range(len(rows))]

    def pooled():
        with ThreadPoolExecutor(threads) as ex:
            return list(ex.map(host, range(len(rows))))

    for name, fn in (("stft_scipy_1t_ms", serial), ("stft_scipy_pool_ms", pooled)):
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            want = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = round(float(np.median(ts[1:])), 3)
    got, _ = down_up()
    got = got.cpu().numpy()
    res["each_equals_scipy"] = all(np.array_equal(got[i], w.astype(np.float64)) for i, w in enumerate(want)
                                   if rows[i][0].dtype == np.float64)
    doc = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
