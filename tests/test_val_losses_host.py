"""CPU: the float64 forms of the validation losses (tests/val_losses_f64.py) against torch's l1_loss on the same images, the defects
the GPU tests (tests/test_gpu_val_losses.py) must be able to see, the mixed-loss weights, the name table of losses.get_loss_function,
the C ABI's declarations, and the refusal rules of validate_list against a stub engine."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import val_losses_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L65 = 28241
BATCH = [1025, 4533, L65]      # the padded batch of the GPU tests, in row order


@pytest.fixture(scope="module")
def pairs():
    return {n: ref.make_pair(n, 100 + i) for i, n in enumerate(BATCH)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the helper against l1_loss
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BATCH)
def test_float64_forms_are_l1_loss_of_the_images(pairs, n):
    est, tgt = pairs[n]
    se, st = torch.from_numpy(ref.magnitude(est)), torch.from_numpy(ref.magnitude(tgt))
    assert se.shape == (ref.frames(n), 1025) and se.dtype == torch.float64
    assert ref.l1_sp(est, tgt) == pytest.approx(float(F.l1_loss(se, st)), rel=1e-13)
    assert ref.l1_log_sp(est, tgt) == pytest.approx(float(F.l1_loss(torch.log10(se), torch.log10(st))), rel=1e-13)
    e64, t64 = torch.from_numpy(est.astype(np.float64)), torch.from_numpy(tgt.astype(np.float64))
    assert ref.l1_wav(est, tgt) == pytest.approx(float(F.l1_loss(e64, t64)), rel=1e-13)
    lg = ref.target_logmel(est)                    # any (frames, 128) image stands in for the model's estimate
    tl = torch.from_numpy(ref.target_logmel(tgt))
    assert tl.shape == (ref.frames(n), 128)
    assert ref.val_l(lg, tgt) == pytest.approx(float(F.l1_loss(torch.from_numpy(lg), tl)), rel=1e-13)
    # the clamp is on the POWER (fDomainHelper.py:62): no magnitude lies below 1e-4, and bins of both clips sit on it
    assert float(se.min()) >= 1e-4 * (1 - 1e-12) and bool((st <= 1.0001e-4).any()) and bool((se <= 1.0001e-4).any())


def test_summation_bound_and_f32_difference():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(5000).astype(np.float32), rng.standard_normal(5000).astype(np.float32)
    mean, bound = ref.mean_abs_f32_diff(a, b)
    exact = float(np.abs((a - b).astype(np.float64)).sum()) / 5000      # (numpy's pairwise sum: far inside the bound)
    assert abs(mean - exact) <= bound and 0 < bound < 1e-11
    assert bound == pytest.approx(5000 * 2.0 ** -53 * mean, rel=1e-12)
    mean, bound = ref.mean_abs_log_diff(np.abs(a) + 1e-4, np.abs(b) + 1e-4)
    assert 0 < bound < 1e-11 and mean > 0.1
    assert ref.mean_abs_f32_diff(a, a) == (0.0, 0.0) and ref.mean_abs_log_diff(np.abs(a) + 1, np.abs(a) + 1)[0] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the defects the GPU tests must see: each moves the value by far more than the bound those tests allow
# ---------------------------------------------------------------------------------------------------------------------------------
def _gpu_bound(n, value):
    """the summation bound of the GPU tests for a clip of n samples whose loss is `value`: n_terms * 2^-53 * sum|terms| / n_terms"""
    return ref.frames(n) * 1025 * 2.0 ** -53 * value + 4 * 2.0 ** -52 * 4.0      # + two ulp64 per logarithm (|log10| <= 4)


@pytest.mark.parametrize("n", BATCH)
def test_planted_defects_move_the_losses(pairs, n):
    est, tgt = pairs[n]
    T, Tmax = ref.frames(n), ref.frames(L65) + (1 if n == L65 else 0)
    sp, lsp = ref.l1_sp(est, tgt), ref.l1_log_sp(est, tgt)
    bound = max(_gpu_bound(n, sp), _gpu_bound(n, lsp))
    assert bound < 1e-10
    moved = {
        "denominator T in place of T_b (l1_sp)": ref.l1_sp(est, tgt, denominator_frames=Tmax) - sp,
        "denominator T in place of T_b (l1_log_sp)": ref.l1_log_sp(est, tgt, denominator_frames=Tmax) - lsp,
        "eps dropped (l1_sp)": ref.l1_sp(est, tgt, eps=0.0) - sp,
        "eps dropped (l1_log_sp)": ref.l1_log_sp(est, tgt, eps=0.0) - lsp,
        "log of the mean (l1_log_sp)": ref.l1_log_sp(est, tgt, log_of_mean=True) - lsp,
        "reflection at Lmax (l1_sp)": ref.l1_sp(est, tgt, row=L65 + 441) - sp,
        "reflection at Lmax (l1_log_sp)": ref.l1_log_sp(est, tgt, row=L65 + 441) - lsp,
    }
    for what, d in moved.items():
        assert abs(d) > 1e4 * bound or not np.isfinite(d), (what, d, bound)
    # val_l: the denominator and the reflection of the target
    lg = ref.target_logmel(est)
    v = ref.val_l(lg, tgt)
    vb = T * 128 * 2.0 ** -53 * v
    assert abs(ref.val_l(lg, tgt, denominator_frames=Tmax) - v) > 1e4 * vb
    assert abs(ref.val_l(lg, tgt, row=L65 + 441) - v) > 1e4 * vb


# ---------------------------------------------------------------------------------------------------------------------------------
# losses.py: weights and names
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mixed_loss_weights():
    from voicefixer_main_amd import losses
    w_wav, w_sp = losses.mix_weights()
    assert w_wav == 0.85 and w_sp == pytest.approx(0.15 / np.sqrt(2048.0), rel=1e-15)
    assert losses.mix_weights(0.5, 1024) == (0.5, 0.5 / 32.0)
    assert ref.mixed(2.0, 3.0) == pytest.approx(w_wav * 2.0 + w_sp * 3.0, rel=1e-15)


class _ColumnsEngine:
    """stands in for Engine: fixed per-clip columns"""
    def __init__(self):
        self.cols = torch.tensor([[1.0, 10.0, 100.0], [3.0, 30.0, 300.0]], dtype=torch.float64)
        self.calls = []

    def spec_losses(self, est, target, lengths=None):
        self.calls.append(("spec_losses", tuple(est.shape), lengths))
        return self.cols

    def l1_rows(self, a, b, counts=None):
        self.calls.append(("l1_rows", tuple(a.shape), counts))
        return self.cols[:, 0]


def test_get_loss_function_names_and_combinations():
    from voicefixer_main_amd import losses
    eng = _ColumnsEngine()
    x = torch.zeros(2, 1, 2000)
    w_wav, w_sp = losses.mix_weights()
    want = {"l1": 2.0, "l1_wav": 2.0, "l1_sp": 20.0, "l1_log_sp": 200.0, "l1_wav_l1_sp": w_wav * 2.0 + w_sp * 20.0,
            "l1_wav_l1_log_sp": w_wav * 2.0 + w_sp * 200.0}
    assert set(want) == set(losses.SUPPORTED)
    for name, v in want.items():
        out = losses.get_loss_function(name, eng)(x, x, lengths=[2000, 1500])
        assert out.dim() == 0 and out.dtype == torch.float64 and float(out) == pytest.approx(v, rel=1e-15), name
    assert all(c[1] == (2, 2000) for c in eng.calls)                       # (B, 1, L) reached the engine as (B, L)
    assert eng.calls[0] == ("l1_rows", (2, 2000), [2000, 1500]) and eng.calls[2] == ("spec_losses", (2, 2000), [2000, 1500])
    # "l1" of tensors that are not waveforms: the flattened rows, lengths counting frames
    eng.calls.clear()
    mel = torch.zeros(2, 1, 7, 128)
    losses.get_loss_function("l1", eng)(mel, mel, lengths=[7, 5])
    assert eng.calls == [("l1_rows", (2, 7, 128), [7 * 128, 5 * 128])]
    with pytest.raises(ValueError, match="waveforms"):
        losses.get_loss_function("l1_sp", eng)(mel, mel)
    with pytest.raises(ValueError, match="differ in shape"):
        losses.get_loss_function("l1", eng)(x, x[:, :, :100])
    # every other name of the reference's table (tools/pytorch/losses.py:52-80) is refused by name
    for name in ("sisnr", "snr", "sispec", "simelspec", "sispeclog", "bce", "wm44k", "lsd"):
        assert name in losses.UNSUPPORTED
        with pytest.raises(NotImplementedError, match="'%s'" % name):
            losses.get_loss_function(name)
    with pytest.raises(ValueError, match="unknown loss"):
        losses.get_loss_function("l2")
    assert "FORWARD VALUES ONLY" in losses.__doc__ and "forward values only" in losses.get_loss_function.__doc__


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI as declared
# ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_bound():
    from voicefixer_main_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vfx.h")).read()
    for name, nargs in (("vfx_spec_losses", 8), ("vfx_validate_gsr_varlen", 10), ("vfx_l1_rows", 8)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define VFX_N_SPEC_LOSSES 3\b", hdr) and _lib.N_SPEC_LOSSES == 3
    mk = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\blosses\.hip\b", mk, re.M)
    # the shared front end is ONE text: stft.hip and losses.hip include it, neither restates the transform
    csrc = os.path.join(ROOT, "voicefixer_main_amd", "csrc")
    for f in ("stft.hip", "losses.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "stft_wave.h"' in src and "void wfft1024(" not in src and "#pragma clang fp contract(off)" in src, f
    src = open(os.path.join(csrc, "losses.hip")).read()
    assert "atomicAdd" not in src and "unsafeAtomicAdd" not in src


# ---------------------------------------------------------------------------------------------------------------------------------
# validate_list against a stub engine
# ---------------------------------------------------------------------------------------------------------------------------------
class _StubEngine:
    hop = 441
    device = torch.device("cpu")

    def __init__(self):
        self.batches = []

    def frames(self, L):
        return L // 441 + 1

    def padded_frames(self, L):
        return -(-self.frames(L) // 64) * 64

    def validate_gsr_varlen(self, x, lengths, t, target_lengths=None):
        assert x.shape == t.shape and x.shape[1] == self.padded_frames(max(lengths)) * 441 - 1
        self.batches.append((list(lengths), list(target_lengths)))
        return torch.tensor([float(n) for n in lengths], dtype=torch.float64)       # a clip's "loss" = its length

    def restore_ssr_varlen(self, x, lengths):
        assert len({self.padded_frames(n) for n in lengths}) == 1                    # one bucket per call
        self.batches.append((list(lengths), None))
        return x

    def spec_losses(self, est, target, lengths=None):
        cols = torch.zeros(len(lengths), 3, dtype=torch.float64)
        cols[:, 1] = torch.tensor([float(n) for n in lengths]) + (0.5 if target is est else 0.0)
        return cols


def _model(cls, eng):
    m = object.__new__(cls)      # (no Engine: the list layer needs hop, device and the two calls only)
    m.engine, m.device = eng, eng.device
    return m


def test_validate_list_order_batches_and_refusals():
    from voicefixer_main_amd import models
    eng = _StubEngine()
    vf = _model(models.VoiceFixer, eng)
    lens = [3000, 30000, 1025, 5000, 2646]
    wavs = [torch.zeros(n) for n in lens]
    tgts = [torch.zeros(n + 3) if n % 441 < 400 else torch.zeros(n) for n in lens]
    per, mean = vf.validate_list(wavs, tgts, max_batch=2)
    assert per == [float(n) for n in lens] and mean == pytest.approx(sum(lens) / 5.0, rel=1e-15)      # input order; the plain mean
    assert [b[0] for b in eng.batches] == [[30000, 5000], [3000, 2646], [1025]]                      # longest first, max_batch each
    assert eng.batches[0][1] == [tgts[1].shape[0], tgts[3].shape[0]]
    with pytest.raises(ValueError, match="2 clips and 1 targets"):
        vf.validate_list(wavs[:2], tgts[:1])
    with pytest.raises(ValueError, match=r"clip 1 has 1024 samples: the STFT needs at least 1025"):
        vf.validate_list([wavs[0], torch.zeros(1024)], [tgts[0], torch.zeros(1024)])
    with pytest.raises(ValueError, match="clip 0 has 7 frames but its target has 8"):
        vf.validate_list([torch.zeros(3000)], [torch.zeros(3100)])
    with pytest.raises(ValueError, match="no clips"):
        vf.validate_list([], [])
    # a clip of 1025 samples (3 frames) is validated although restore_scored_list refuses it (no SSIM here)
    with pytest.raises(ValueError, match="the scores need at least 2646"):
        list(models._paired_batches(eng, [torch.zeros(1025)], [torch.zeros(1025)], 4, lambda L: 0, lambda L: L, "x",
                                    models.MIN_SCORED_SAMPLES, ("the scores need", "7 STFT frames")))

    # SSR_UNet: equal lengths, one padded-frame bucket per call, the reference chosen by `against`
    eng = _StubEngine()
    ssr = _model(models.SSR_UNet, eng)
    assert models.GSR_UNet is models.SSR_UNet
    wavs = [torch.zeros(n) for n in lens]
    per, mean = ssr.validate_list(wavs, [torch.zeros(n) for n in lens], max_batch=16)
    assert per == [float(n) for n in lens]
    assert [b[0] for b in eng.batches] == [[30000], [5000, 3000, 2646, 1025]]
    per_in, _ = ssr.validate_list(wavs, [torch.zeros(n) for n in lens], against="input")
    assert per_in == [n + 0.5 for n in lens]                                    # compared with the restored input's own row
    with pytest.raises(ValueError, match="clip 0 has 3000 samples but its target has 3003"):
        ssr.validate_list(wavs[:1], [torch.zeros(3003)])
    with pytest.raises(ValueError, match="against must be one of"):
        ssr.validate_list(wavs, wavs, against="sp_target")
    doc = models.SSR_UNet.validation_step.__doc__
    assert "ssr_unet.py:232" in doc and "not reproduced" in doc and "gsr_unet.py:230" in doc
