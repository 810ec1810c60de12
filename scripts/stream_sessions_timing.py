#!/usr/bin/env python3
"""What one step of a streaming session costs (voicefixer_main_amd/streaming.py, csrc/stream.hip) on an MI355X.

A session of S slots in overlap-add mode, W = 44100, hop W / 2, Hann window; every slot is fed one hop per step, so exactly one
chunk per slot falls due and the step is: push (S blocks, already on the device, as one packed buffer) -> next (gather S rows) ->
the network on the (S, 1, W) batch -> put (stitch) -> pop.  Timed is `StreamRestorer.feed` as a caller sees it -- a host clock around
the call and a device synchronise, median of --reps after --warmup steps -- for S = 1, 16, 64 and two networks:

  toy      the stand-in of the chunker tests (three element-wise launches): the session's own cost
  restore  VoiceFixer.restore on synthetic weights, precision 2 (what bench.py runs)

and beside each the same batch through the offline pair, `Engine.chunk_gather` + the network + `Engine.chunk_ola` on an (S, W)
signal (code this session feature does not touch).  `launches` is what the session itself enqueues per step (push, gather, stitch,
pop; tables of 64 rows, 32 slots for the overlap-add stitch), counted from the table sizes.

Every configuration runs in a child process of its own under its own time limit; the first that fails ends the run.

    python scripts/stream_sessions_timing.py [--reps=20] [--warmup=3] [--out=profiles/stream_sessions.json]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = 44100
H = W // 2
LIMIT_S = {"toy": 120, "restore": 300}


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def toy_net(x):
    import torch
    prev = torch.cat([torch.zeros_like(x[..., :1]), x[..., :-1]], -1)
    n = x.shape[-1]
    ramp = (torch.arange(n, dtype=torch.float32, device=x.device) / n) * 0.05
    return {"wav": 0.6 * x + 0.3 * prev + ramp}


def one(net, S, reps, warmup):
    import numpy as np
    import torch
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.chunker import _window
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_VOCODER
    from voicefixer_main_amd.streaming import StreamRestorer
    if not torch.cuda.is_available():
        raise SystemExit("stream_sessions_timing: no GPU")
    if net == "toy":
        eng = Engine("cuda:0")
        nnet = toy_net
    else:
        from voicefixer_main_amd.models import VoiceFixer
        eng = Engine("cuda:0", config={"precision": 2})
        unet_sd, voc_sd = synth.make_resunet_state_dict(0), synth.make_vocoder_state_dict(1)
        eng.load_state_dict(MODEL_UNET_MEL, unet_sd)
        eng.load_state_dict(MODEL_VOCODER, voc_sd)
        vf = VoiceFixer(None, channels=2, type_target="vocals", engine=eng)
        sd = {"generator.analysis_module." + k: v for k, v in unet_sd.items()}
        sd.update({"vocoder.model." + k: v for k, v in voc_sd.items()})
        vf.load_state_dict(sd)
        vf = vf.eval().to(torch.device("cuda:0"))
        nnet = lambda c: {"wav": vf.restore(c)}   # noqa: E731
    steps = warmup + reps
    audio = torch.from_numpy(synth.make_clips(1, (steps + 2) * H / 44100.0 + 0.1, seed=7)).cuda()[0, 0]
    r = StreamRestorer(nnet, W, hop_size=H, window="hanning", slots=S, max_batch=64, engine=eng)
    slots = [r.open() for _ in range(S)]
    r.feed({s: audio[:H] for s in slots})          # chunk 1: mostly the zeros in front of the stream
    ms = []
    for t in range(1, steps + 1):
        blocks = {s: audio[t * H:(t + 1) * H] for s in slots}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = r.feed(blocks)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert all(got[s].numel() == H for s in slots)
    # the same batch through the offline pair: S chunks of W, one per row
    x = audio[:W].repeat(S, 1).contiguous()
    win = torch.from_numpy(_window("hanning", W)).cuda()
    ref = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chunks = eng.chunk_gather(x, W, W, 0, 1)
        frames = nnet(chunks.view(S, 1, W))["wav"].reshape(S, 1, W)
        eng.chunk_ola(frames, win, 0.5, W, 0, W)
        torch.cuda.synchronize()
        ref.append((time.perf_counter() - t0) * 1e3)
    rows = lambda n, per: -(-n // per)   # noqa: E731
    return {"net": net, "slots": S, "window_size": W, "hop_size": H, "reps": reps, "warmup": warmup,
            "step_ms": round(float(np.median(ms[warmup:])), 4), "step_ms_min": round(min(ms[warmup:]), 4),
            "step_ms_max": round(max(ms[warmup:]), 4),
            "offline_pair_ms": round(float(np.median(ref[warmup:])), 4), "offline_pair_ms_min": round(min(ref[warmup:]), 4),
            "launches": {"push": rows(S, 64), "gather": rows(S, 64), "stitch": rows(S, 32), "pop": rows(S, 64)},
            "device": torch.cuda.get_device_name(0)}


def main():
    reps, warmup = opt("reps", 20, int), opt("warmup", 3, int)
    only = opt("one", "", str)
    if only:      # a child: one configuration, one JSON line
        net, S = only.split(",")
        print(json.dumps(one(net, int(S), reps, warmup)))
        return
    out_path = opt("out", os.path.join(ROOT, "profiles", "stream_sessions.json"), str)
    results = []
    for net in ("toy", "restore"):
        for S in (1, 16, 64):
            cmd = [sys.executable, os.path.abspath(__file__), "--one=%s,%d" % (net, S), "--reps=%d" % reps, "--warmup=%d" % warmup]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[net])
            except subprocess.TimeoutExpired:
                raise SystemExit("stream_sessions_timing: %s with %d slots ran past its %d s" % (net, S, LIMIT_S[net]))
            lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not lines:      # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("stream_sessions_timing: %s with %d slots failed (exit status %d)" % (net, S, p.returncode))
            results.append(json.loads(lines[-1]))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps({"what": "one step of a streaming session, one chunk due per slot; see scripts/stream_sessions_timing.py",
                            "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
