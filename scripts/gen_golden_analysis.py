#!/usr/bin/env python3
"""Write tests/golden/gsr_analysis.npz: the bi_gru and dnn analysis modules of the REFERENCE's own Generator
(models/gsr_voicefixer.py:14-91, imported unmodified) on the seeded state_dicts of voicefixer_main_amd.synth.

The state_dicts are stored as keys, shapes and per-tensor fingerprints (fingerprint()); the inputs and outputs in full.
The module's imports that do not exist offline are stubbed in sys.modules before it is imported: `voicefixer` (the vocoder
package), `pytorch_lightning`, and the `tools.*` / `dataloaders.*` star imports -- Generator.forward needs nothing of them but
`to_log`, which comes from the reference's own tools/pytorch/pytorch_util.py.  Needs a checkout of the reference (--ref);
runs on the CPU, in float32 and float64.

    python scripts/gen_golden_analysis.py --ref <path to the reference checkout>
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voicefixer_main_amd import synth  # noqa: E402

SWITCHES = ("unet", "unet_small", "bi_gru", "dnn")


def import_reference_generator(ref):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Module(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

    stub("voicefixer", Vocoder=_Module)
    pl = stub("pytorch_lightning", LightningModule=_Module)
    spec = importlib.util.spec_from_file_location("ref_pytorch_util", os.path.join(ref, "tools", "pytorch", "pytorch_util.py"))
    pu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pu)
    common = dict(torch=torch, nn=torch.nn, np=np, os=os, pl=pl)
    for name in ("tools", "tools.pytorch", "tools.callbacks", "tools.file", "dataloaders", "dataloaders.augmentation"):
        stub(name)
    stub("tools.pytorch.mel_scale", MelScale=_Module)
    stub("tools.callbacks.base", **common)
    stub("tools.pytorch.losses", **common)
    stub("tools.pytorch.pytorch_util", **common, to_log=pu.to_log, from_log=pu.from_log)
    stub("tools.pytorch.random_", **common)
    stub("tools.file.wav", **common)
    stub("dataloaders.augmentation.base", add_noise_and_scale_with_HQ_with_Aug=None)
    stub("tools.utils", trim_center=None)
    spec = importlib.util.spec_from_file_location("ref_gsr_voicefixer", os.path.join(ref, "models", "gsr_voicefixer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Generator


def fingerprint(v):
    """sum, sum of squares and the first 8 values (float64) of a tensor: what tests/golden pins the synth state_dicts by."""
    a = v.detach().double().reshape(-1).numpy()
    head = np.zeros(8)
    head[:min(8, a.size)] = a[:8]
    return np.concatenate([[a.sum(), (a * a).sum()], head])


def hp_for(module):
    return {"task": {"gsr": {"gsr_model": {"voicefixer": {s: s == module for s in SWITCHES}}}},
            "model": {"mel_freq_bins": 128, "channels_in": 1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gsr_analysis.npz"))
    args = ap.parse_args()
    Generator = import_reference_generator(args.ref)
    out = {}
    rng = np.random.default_rng(20260)
    inputs = {}
    for T in (37, 101):
        # linear mel whose log10 spans the front-end's range (-8 .. 2), exact zeros included (to_log's clip)
        lg = rng.uniform(-7.5, 1.5, size=(2, 1, T, 128))
        mel = (10.0 ** lg).astype(np.float32)
        mel[0, 0, 3, :5] = 0.0
        inputs[T] = mel
        out["mel_T%d" % T] = mel
    for module, make in (("bi_gru", synth.make_gru_analysis_state_dict), ("dnn", synth.make_dnn_analysis_state_dict)):
        sd = make()
        gen = Generator(hp_for(module)).eval()
        gen.analysis_module.load_state_dict(sd, strict=True)
        ref_sd = gen.analysis_module.state_dict()
        assert list(ref_sd.keys()) == list(sd.keys()), (module, list(ref_sd.keys()), list(sd.keys()))
        out["%s_keys" % module] = np.array(list(sd.keys()))
        for k, v in sd.items():
            # the tensors themselves are synth's (seeded, 20 MB together): the fixture pins them by a fingerprint
            out["%s_fp/%s" % (module, k)] = fingerprint(v)
            out["%s_shape/%s" % (module, k)] = np.array(tuple(v.shape), dtype=np.int64)
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            g = gen.to(dt)
            with torch.no_grad():
                for T, mel in inputs.items():
                    y = g(torch.from_numpy(mel).to(dt))["mel"]
                    out["%s_out_T%d_%s" % (module, T, tag)] = y.numpy()
        print(module, "ok:", len(sd), "tensors")
    np.savez_compressed(args.out, **out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
