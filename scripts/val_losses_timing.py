#!/usr/bin/env python3
"""The validation losses at 16 clips of 10 s, each against the path it replaces, in one process:

  (a) spec_losses_ms      ONE Engine.spec_losses call (the waveform L1, the fused pair-STFT L1 launch, the final kernel) between HIP
                          events, after warm-up calls, median of --reps
      two_launch_ms       what it replaces: two vfx_stft_phase calls that write both (16, 1001, 1025) magnitude images, torch's
                          l1_loss of the images, of their log10 and of the waveforms -- timed the same way, alternating with (a)
  (b) validate_list_ms    VoiceFixer.validate_list on the 16 files (host lists in, floats out), wall time with a device
                          synchronisation, median of --reps
      scored_list_ms      VoiceFixer.restore_scored_list on the same files: the restore with the vocoder and the handler scores,
                          the only route to a per-file number before validate_list -- alternating with (b)
  sclk_mhz                the shader clock read from hwmon while the timed calls ran

Seeded synthetic weights (precision 1) and speech-like clips.  Writes one JSON line to profiles/val_losses_timing.json (or --out=).
Run it under one time limit:

    timeout -k 10 600 python scripts/val_losses_timing.py [--reps=9] [--out=profiles/val_losses_timing.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import PowerSampler  # noqa: E402
from voicefixer_main_amd import synth  # noqa: E402
from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_VOCODER  # noqa: E402
from voicefixer_main_amd.models import VoiceFixer  # noqa: E402

FS = 44100


def opt(name, default, cast=float):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return cast(v[0]) if v else default


def alternate(fa, fb, reps, device, events):
    """median ms of fa and of fb, called in turn (a, b, a, b, ...) after two warm-up rounds"""
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize(device)
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            if events:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                torch.cuda.synchronize(device)
                ts.append(a.elapsed_time(b))
            else:
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(device)
                ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ta)), float(np.median(tb))


def main():
    reps = opt("reps", 9, int)
    clips_n, seconds = opt("clips", 16, int), opt("seconds", 10.0)
    out_path = opt("out", os.path.join(ROOT, "profiles", "val_losses_timing.json"), str)
    if not torch.cuda.is_available():
        raise SystemExit("val_losses_timing: no GPU")
    eng = Engine("cuda:0", config={"precision": 1})
    eng.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
    eng.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
    model = VoiceFixer(engine=eng)
    n = int(seconds * FS)
    clean = [(synth.speech_like(n, 40 + i) * 0.6).astype(np.float32) for i in range(clips_n)]
    noisy = [synth.degrade(c, 40 + i)[:n].astype(np.float32) for i, c in enumerate(clean)]
    est = torch.from_numpy(np.stack(noisy)).to(eng.device)
    tgt = torch.from_numpy(np.stack(clean)).to(eng.device)

    def two_launch():
        se = eng.stft(est, want_mel=False, want_sp=True, eps=1.0000001e-8)["sp"]      # (an eps other than 1e-8: vfx_stft_phase)
        st = eng.stft(tgt, want_mel=False, want_sp=True, eps=1.0000001e-8)["sp"]
        return F.l1_loss(est, tgt), F.l1_loss(se, st), F.l1_loss(torch.log10(se), torch.log10(st))

    fused = lambda: eng.spec_losses(est, tgt)
    wavs, tgts = [torch.from_numpy(x) for x in noisy], [torch.from_numpy(x) for x in clean]
    with PowerSampler() as ps:
        a_ms, a_ref_ms = alternate(fused, two_launch, reps, eng.device, events=True)
        b_ms, b_ref_ms = alternate(lambda: model.validate_list(wavs, tgts), lambda: model.restore_scored_list(wavs, tgts), reps,
                                   eng.device, events=False)
    power = ps.result() or {}
    cols = fused().mean(dim=0).cpu().tolist()
    ref = [float(v) for v in two_launch()]
    res = {"clips": clips_n, "seconds_each": seconds, "reps": reps, "device": torch.cuda.get_device_name(0),
           "spec_losses_ms": round(a_ms, 4), "two_launch_ms": round(a_ref_ms, 4), "two_launch_over_spec_losses": round(a_ref_ms / a_ms, 2),
           "validate_list_ms": round(b_ms, 3), "scored_list_ms": round(b_ref_ms, 3), "scored_over_validate": round(b_ref_ms / b_ms, 2),
           "spec_losses_batch_mean": cols, "two_launch_values": ref,
           "sclk_mhz": power.get("avg_sclk_mhz"), "min_sclk_mhz": power.get("min_sclk_mhz")}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
