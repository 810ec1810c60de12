"""CPU tests of the bi_gru / dnn analysis modules (models/gsr_voicefixer.py:44-91): the synthetic state_dicts against the
reference's own module (tests/golden/gsr_analysis.npz, scripts/gen_golden_analysis.py), the float64 restatement the GPU tests
compare against, the module selection of models.VoiceFixer, and the static assembly checks of csrc/analysis.hip."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from voicefixer_main_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "gsr_analysis.npz")
MAKERS = {"bi_gru": synth.make_gru_analysis_state_dict, "dnn": synth.make_dnn_analysis_state_dict}


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatement of Generator.forward with the bi_gru / dnn module (eval mode); the GPU tests import it
# ----------------------------------------------------------------------------------------------------------------------
def _bn(sd, p, x):
    g, b = sd[p + ".weight"].double(), sd[p + ".bias"].double()
    mu, var = sd[p + ".running_mean"].double(), sd[p + ".running_var"].double()
    return g * (x - mu) / torch.sqrt(var + 1e-5) + b


def _linear(sd, p, x):
    return torch.nn.functional.linear(x, sd[p + ".weight"].double(), sd[p + ".bias"].double())


def reference_forward(module, sd, mel, frames=None):
    """mel (B, T, 128) linear -> log-mel estimate (B, T, 128) in float64, analysis(to_log(mel)) + to_log(mel).  With `frames`,
    clip b is its own first frames[b] rows (rows past them zero)."""
    mel = torch.as_tensor(np.asarray(mel)).double()
    if frames is not None:
        out = torch.zeros_like(mel)
        for b, n in enumerate(frames):
            out[b, :n] = torch.from_numpy(reference_forward(module, sd, mel[b:b + 1, :n])[0])
        return out.numpy()
    assert (mel >= 0).all()
    x = torch.log10(torch.clip(mel, min=1e-8))
    if module == "bi_gru":
        h = _bn(sd, "2.bn", _linear(sd, "1", _bn(sd, "0", x)))
        gru = torch.nn.GRU(256, 256, num_layers=2, bidirectional=True, batch_first=True).double()
        gru.load_state_dict({k[len("2.gru."):]: v.double() for k, v in sd.items() if k.startswith("2.gru.")})
        with torch.no_grad():
            h, _ = gru(h)
        y = _linear(sd, "6", torch.relu(_linear(sd, "4", torch.relu(h))))
    else:
        h = x
        for i, p in enumerate((0, 3, 6, 9, 12)):
            h = torch.relu(_linear(sd, str(p), h))
            if i < 4:
                h = _bn(sd, str(p + 2), h)
        y = _linear(sd, "14", h)
    return (y + x).detach().numpy()


def _fingerprint(v):
    a = v.detach().double().reshape(-1).numpy()
    head = np.zeros(8)
    head[:min(8, a.size)] = a[:8]
    return np.concatenate([[a.sum(), (a * a).sum()], head])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("module", ["bi_gru", "dnn"])
def test_synth_state_dict_matches_reference_keys_shapes_and_tensors(golden, module):
    sd = MAKERS[module]()
    assert list(sd.keys()) == [str(k) for k in golden["%s_keys" % module]]
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(golden["%s_shape/%s" % (module, k)]), k
        np.testing.assert_allclose(_fingerprint(v), golden["%s_fp/%s" % (module, k)], rtol=1e-12, atol=1e-12, err_msg=k)
    # non-zero biases everywhere (b_hn included): a bias added in the wrong place must change the result
    for k, v in sd.items():
        if "bias" in k and "running" not in k:
            assert float(v.abs().min()) > 0.0, k


@pytest.mark.parametrize("module", ["bi_gru", "dnn"])
@pytest.mark.parametrize("T", [37, 101])
def test_float64_restatement_reproduces_reference_module(golden, module, T):
    sd = MAKERS[module]()
    mel = golden["mel_T%d" % T][:, 0]
    ours = reference_forward(module, sd, mel)
    ref64 = golden["%s_out_T%d_f64" % (module, T)][:, 0]
    np.testing.assert_allclose(ours, ref64, rtol=0, atol=1e-10)
    # the reference in float32 sits within fp32 rounding of it (the bar the fp32 kernels are held to is coarser)
    assert np.abs(golden["%s_out_T%d_f32" % (module, T)][:, 0] - ref64).max() < 1e-4


def test_restatement_frames_are_independent_clips(golden):
    sd = MAKERS["bi_gru"]()
    mel = golden["mel_T37"][:, 0]
    full = reference_forward("bi_gru", sd, mel, frames=[37, 20])
    np.testing.assert_allclose(full[1, :20], reference_forward("bi_gru", sd, mel[1:2, :20])[0], atol=1e-12)
    assert (full[1, 20:] == 0).all()
    # a backward pass that started at the padded end would differ
    assert np.abs(full[1, :20] - reference_forward("bi_gru", sd, mel[1:2])[0, :20]).max() > 1e-3


# ----------------------------------------------------------------------------------------------------------------------
# module selection (models.VoiceFixer, pure functions: no GPU)
# ----------------------------------------------------------------------------------------------------------------------
def _hp(switch, n_mel=128):
    sw = {s: s == switch for s in ("unet", "unet_small", "bi_gru", "dnn")}
    return {"task": {"gsr": {"gsr_model": {"voicefixer": sw}}}, "model": {"mel_freq_bins": n_mel}}


def _keys(module, prefix="generator.analysis_module."):
    if module == "unet":
        return [prefix + k for k, _ in synth.resunet_layout()]
    return [prefix + k for k in MAKERS[module]()] + ["vocoder.model.condnet.0.weight"]


def test_module_from_keys():
    from voicefixer_main_amd.models import analysis_module_from_keys
    assert analysis_module_from_keys(_keys("bi_gru")) == "bi_gru"
    assert analysis_module_from_keys(_keys("dnn")) == "dnn"
    assert analysis_module_from_keys(_keys("unet")) == "unet"
    assert analysis_module_from_keys([k.split("analysis_module.")[1] for k in _keys("dnn") if "analysis_module." in k]) == "dnn"
    assert analysis_module_from_keys(["vocoder.model.condnet.0.weight"]) is None


def test_module_from_hp_switches():
    from voicefixer_main_amd.models import analysis_module_from_hp
    for s, want in (("unet", "unet"), ("unet_small", "unet"), ("bi_gru", "bi_gru"), ("dnn", "dnn")):
        assert analysis_module_from_hp(_hp(s)) == want
    assert analysis_module_from_hp({"model": {}}) is None
    with pytest.raises(ValueError, match="mel_freq_bins"):
        analysis_module_from_hp(_hp("bi_gru", n_mel=80))
    assert analysis_module_from_hp(_hp("none")) is None


def test_selection_cross_checks_hp_and_checkpoint_hp():
    from voicefixer_main_amd.models import select_analysis_module
    assert select_analysis_module(_keys("bi_gru"), _hp("bi_gru"), _hp("bi_gru")) == "bi_gru"
    assert select_analysis_module(_keys("unet"), _hp("unet_small")) == "unet"
    assert select_analysis_module(_keys("dnn"), None, None) == "dnn"
    with pytest.raises(ValueError, match="'dnn'.*'bi_gru'"):
        select_analysis_module(_keys("bi_gru"), _hp("dnn"))
    with pytest.raises(ValueError, match="checkpoint.*'unet'.*'dnn'"):
        select_analysis_module(_keys("dnn"), _hp("dnn"), _hp("unet"))


def test_library_exports_the_analysis_entry_points():
    from voicefixer_main_amd import _lib
    assert (_lib.MODEL_GRU_MEL, _lib.MODEL_DNN_MEL) == (4, 5)
    hdr = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert re.search(r"VFX_MODEL_GRU_MEL = 4", hdr) and re.search(r"VFX_MODEL_DNN_MEL = 5", hdr)
    for name in ("vfx_analysis_mel", "vfx_select_analysis"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, hdr)


# ----------------------------------------------------------------------------------------------------------------------
# analysis.hip on gfx950: no spills, no FLAT memory operations, clean under both assembly checkers
# ----------------------------------------------------------------------------------------------------------------------
def test_analysis_kernels_assembly_is_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "analysis.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", out, os.path.join(ROOT, "voicefixer_main_amd", "csrc", "analysis.hip")],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    kernels = dict(re.findall(r"\n(_ZN3vfx\w+):.*?; ScratchSize: (\d+)", asm, re.S))
    assert any("k_gru_seq" in k for k in kernels) and any("k_dense" in k for k in kernels), list(kernels)
    for k, scratch in kernels.items():
        assert int(scratch) == 0, (k, scratch)
    assert not re.search(r"\n\s*flat_(load|store|atomic)", asm)
    for checker in ("asm_store_hazard_check.py", "asm_inflight_check.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", checker), out], capture_output=True, text=True)
        assert r.returncode == 0, (checker, r.stdout[-2000:])
