"""GPU: the validation losses on the device (csrc/losses.hip: k_pair_stft_l1, k_l1_rows, k_loss_final) -- vfx_spec_losses against
float64 host sums over the device's own vfx_stft_phase magnitudes and over the samples, vfx_validate_gsr_varlen against
vfx_restore_gsr_varlen's log-mel and vfx_stft_mel's target log-mel for each analysis module, batch independence with == on the doubles,
the refusals, and the Python surface (Engine, losses.get_loss_function, VoiceFixer / SSR_UNet validation_step and validate_list).

Every bound is the summation bound of tests/val_losses_f64.py (n 2^-53 sum|terms|, two ulp64 per logarithm on top for the log column),
computed by the test from the terms themselves; tests/test_val_losses_host.py shows that the defects a padded-batch implementation can
have move the values by more than 10^4 times as much.

As measured on an MI355X: |device - host| is 0.0 in every case of columns 0 and 1 and of val_l, and at most 5.6e-17 (one ulp of the
value) in the log column, against bounds of 5e-17 .. 3e-12."""
import ctypes

import numpy as np
import pytest
import torch

import val_losses_f64 as ref
from frontend_f64 import EDGE_LENGTHS, L65

pytestmark = pytest.mark.gpu

HOP = 441
BATCH = [1025, 4533, L65]            # one padded batch, in this row order: 3, 11 and 65 frames (a 64-frame pad is crossed)
BATCH_T = [1100, 4600, 28300]        # the targets' own lengths for val_l: the same frame counts
MODULES = ("unet", "bi_gru", "dnn")


@pytest.fixture(scope="module")
def engines():
    """(a handle with the three analysis modules and the spectrogram ResUNet and NO vocoder, one with the same weights and a vocoder)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.engine import Engine, MODEL_DNN_MEL, MODEL_GRU_MEL, MODEL_UNET_MEL, MODEL_UNET_SPEC, MODEL_VOCODER
    out = []
    for with_voc in (False, True):
        e = Engine("cuda:0", config={"precision": 1})
        e.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
        e.load_state_dict(MODEL_GRU_MEL, synth.make_gru_analysis_state_dict())
        e.load_state_dict(MODEL_DNN_MEL, synth.make_dnn_analysis_state_dict())
        if with_voc:
            e.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
        else:
            e.load_state_dict(MODEL_UNET_SPEC, synth.make_resunet_state_dict(2))
        out.append(e)
    return tuple(out)


@pytest.fixture(scope="module")
def eng(engines):
    return engines[0]


def _mid(module):
    from voicefixer_main_amd.models import ANALYSIS_MODEL_IDS
    return ANALYSIS_MODEL_IDS[module]


def _pad(clips, width):
    x = torch.zeros(len(clips), width)
    for b, c in enumerate(clips):
        x[b, :len(c)] = torch.from_numpy(np.asarray(c))
    return x


def _sp(eng, clip):
    """the device's own vfx_stft_phase(eps = 1e-8) magnitudes of one clip alone -> (T, 1025) float32"""
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import _ptr
    x = torch.from_numpy(np.asarray(clip))[None].to(eng.device).contiguous()
    sp = torch.empty((1, eng.frames(x.shape[1]), 1025), device=eng.device, dtype=torch.float32)
    _lib.check(eng.lib.vfx_stft_phase(eng.h, _ptr(x), 1, x.shape[1], _ptr(sp), None, None, ctypes.c_float(1e-8), eng._stream()),
               "vfx_stft_phase")
    return sp[0].cpu().numpy()


@pytest.fixture(scope="module")
def pairs():
    """{n: (est, target)} of every clip length of this file, computed once"""
    return {n: ref.make_pair(n, 100 + i) for i, n in enumerate(sorted(set(EDGE_LENGTHS + BATCH)))}


@pytest.fixture(scope="module")
def many():
    """130 pairs of 1025 .. 1323 samples (3 or 4 frames): one more than a sub-batch of 128 clips, and then one"""
    rng = np.random.default_rng(3)
    lens = [int(v) for v in rng.integers(1025, 1324, size=130)]
    lens[0], lens[127], lens[128], lens[129] = 1323, 1025, 1322, 1323
    return lens, [ref.make_pair(n, 500 + i) for i, n in enumerate(lens)]


# ---------------------------------------------------------------------------------------------------------------------------------
# vfx_spec_losses
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(set(EDGE_LENGTHS + [L65])))
def test_spec_losses_single_clip_vs_host_sums(eng, pairs, n):
    """Columns 1 and 2 against float64 host sums over the device's own magnitudes (bit-identical magnitudes AND the summation in one
    check), column 0 against the host sum over the samples."""
    est, tgt = pairs[n]
    got = eng.spec_losses(est[None], tgt[None]).cpu().numpy()
    assert got.shape == (1, 3) and got.dtype == np.float64
    se, st = _sp(eng, est), _sp(eng, tgt)
    assert se.shape == (n // HOP + 1, 1025)
    want = [ref.mean_abs_f32_diff(est, tgt), ref.mean_abs_f32_diff(se, st), ref.mean_abs_log_diff(se, st)]
    for col, (value, bound) in enumerate(want):
        print("n", n, "column", col, "device", got[0, col], "host", value, "|difference|", abs(got[0, col] - value), "bound", bound)
    for col, (value, bound) in enumerate(want):
        assert value > 0 and bound < 1e-9 * value
        assert abs(got[0, col] - value) <= bound, (n, col, got[0, col], value, bound)
    # and the float64 oracle.  Column 0: the float32 subtraction rounds every term by at most 2^-24 of itself.  Column 1: the oracle's
    # STFT is float64, the device's float32 -- a radix-2-equivalent transform of 2048 points errs by at most 11 * 2^-24 * sum|x w| <=
    # 11 * 6e-8 * (1.2 AMP * 1024) per bin, twice that per difference (the log column, where a bin at the clamp turns this into a
    # relative error of its own size, has no such bound and is not compared)
    assert got[0, 0] == pytest.approx(ref.l1_wav(est, tgt), rel=2.0 ** -23)
    assert abs(got[0, 1] - ref.l1_sp(est, tgt)) <= 2 * 11 * 6e-8 * 1.2 * ref.AMP * 1024


def test_spec_losses_identical_pair_is_exactly_zero(eng, pairs):
    x = _pad([pairs[n][1] for n in BATCH], L65 + 300)
    got = eng.spec_losses(x, x.clone(), BATCH).cpu()
    assert got.shape == (3, 3) and torch.equal(got, torch.zeros(3, 3, dtype=torch.float64))
    one = torch.from_numpy(pairs[2048][0])
    assert torch.equal(eng.spec_losses(one, one.clone()).cpu(), torch.zeros(1, 3, dtype=torch.float64))       # (L,) -> (1, 3)


def _alone(eng, est, tgt):
    return eng.spec_losses(est[None], tgt[None]).cpu()[0]


def test_spec_losses_padded_batch_equals_own_call(eng, pairs):
    """every clip of the padded batch == its own B = 1 call at its own length, whatever lies past its end in its row"""
    Lmax = L65 + 300
    est, tgt = _pad([pairs[n][0] for n in BATCH], Lmax), _pad([pairs[n][1] for n in BATCH], Lmax)
    for b, n in enumerate(BATCH):        # what lies past a clip's end is never read
        est[b, n:] = 7.0
        tgt[b, n:] = float("nan")
    got = eng.spec_losses(est, tgt, BATCH).cpu()
    assert torch.isfinite(got).all() and (got > 0).all()
    for b, n in enumerate(BATCH):
        assert torch.equal(got[b], _alone(eng, *pairs[n])), (b, got[b], _alone(eng, *pairs[n]))
    # lengths = None: every clip has Lmax samples
    full = eng.spec_losses(est[2:, :L65], tgt[2:, :L65]).cpu()
    assert torch.equal(full[0], got[2])


def test_spec_losses_130_clips_cross_the_sub_batch(eng, many):
    lens, prs = many
    Lmax = max(lens)
    est, tgt = _pad([p[0] for p in prs], Lmax), _pad([p[1] for p in prs], Lmax)
    got = eng.spec_losses(est, tgt, lens).cpu()
    assert got.shape == (130, 3) and torch.isfinite(got).all()
    for b in (0, 1, 63, 64, 126, 127, 128, 129):
        assert torch.equal(got[b], _alone(eng, *prs[b])), b
    # the same clips in another order and another batch: a clip's numbers depend on the clip alone
    perm = list(range(129, -1, -1))
    again = eng.spec_losses(est[perm][:70], tgt[perm][:70], [lens[i] for i in perm[:70]]).cpu()
    assert torch.equal(again, got[perm][:70])


def test_spec_losses_one_changed_sample(eng, pairs):
    """est = target but for ONE sample: l1_wav = |delta| / L, and l1_sp comes from the frames that contain the sample alone"""
    n, k = L65, 14000
    tgt = pairs[n][1]
    est = tgt.copy()
    est[k] = np.float32(est[k] + np.float32(0.01))
    delta = float(np.abs(np.float32(est[k] - tgt[k])))
    got = eng.spec_losses(est[None], tgt[None]).cpu().numpy()[0]
    assert delta > 0 and abs(got[0] - delta / n) <= n * 2.0 ** -53 * (delta / n)
    se, st = _sp(eng, est), _sp(eng, tgt)
    per_frame = np.abs(se - st).astype(np.float64).sum(axis=1)
    holds = np.array([t * HOP - 1024 <= k < t * HOP + 1024 for t in range(n // HOP + 1)])      # (k is far from both reflections)
    assert holds.sum() == 5 and (per_frame[holds] > 0).all() and (per_frame[~holds] == 0).all()
    value, bound = ref.mean_abs_f32_diff(se, st)
    assert abs(got[1] - value) <= bound and abs(value - per_frame[holds].sum() / (per_frame.size * 1025)) <= bound
    assert got[2] > 0


def test_spec_losses_refusals_launch_nothing(eng, pairs):
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import _ptr
    x = _pad([pairs[n][0] for n in BATCH], L65).to(eng.device)
    out = torch.full((3, 3), -7.0, device=eng.device, dtype=torch.float64)
    call = lambda e, t, B, L, lens, o: eng.lib.vfx_spec_losses(eng.h, e, t, B, L, lens, o, eng._stream())
    arr = lambda v: (ctypes.c_int * len(v))(*v)
    cases = [
        ((None, _ptr(x), 3, L65, arr(BATCH), _ptr(out)), "NULL"),
        ((_ptr(x), None, 3, L65, arr(BATCH), _ptr(out)), "NULL"),
        ((_ptr(x), _ptr(x), 3, L65, arr(BATCH), None), "NULL"),
        ((_ptr(x), _ptr(x), 0, L65, arr(BATCH), _ptr(out)), "B > 0"),
    ]
    for args, text in cases:
        rc = call(*args)
        assert rc == 1 and text in eng.lib.vfx_last_error().decode(), (rc, eng.lib.vfx_last_error())
    for lens, clip in (([1025, 1024, L65], 1), ([1025, 4533, L65 + 1], 2), ([-1, 4533, L65], 0)):
        with pytest.raises(RuntimeError, match=r"vfx_spec_losses: clip %d has %d samples" % (clip, lens[clip])):
            eng.spec_losses(x, x, lens)
    with pytest.raises(RuntimeError, match="clip 0 has 1000 samples"):
        eng.spec_losses(x[:, :1000], x[:, :1000])
    with pytest.raises(ValueError, match="2 lengths for 3 clips"):
        eng.spec_losses(x, x, [1025, 1025])
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((3, 3), -7.0, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# vfx_validate_gsr_varlen
# ---------------------------------------------------------------------------------------------------------------------------------
def _val_batch(eng):
    """(noisy (3, Lmax), targets (3, Lmax), Lmax): the targets have their own lengths and sample values past the clips' ends"""
    Lmax = eng.padded_frames(max(BATCH)) * HOP - 1
    prs = [ref.make_pair(m, 300 + b) for b, m in enumerate(BATCH_T)]
    return _pad([p[0][:n] * 50.0 for p, n in zip(prs, BATCH)], Lmax), _pad([p[1] * 50.0 for p in prs], Lmax), Lmax


@pytest.mark.parametrize("module", MODULES)
def test_validate_gsr_varlen(engines, module):
    eng, full = engines
    eng.select_analysis(_mid(module))
    full.select_analysis(_mid(module))
    try:
        wav, tgt, Lmax = _val_batch(eng)
        val, logmel = eng.validate_gsr_varlen(wav, BATCH, tgt, BATCH_T, want_logmel=True)
        val, logmel = val.cpu(), logmel.cpu()
        assert val.shape == (3,) and val.dtype == torch.float64 and torch.isfinite(val).all()
        # this handle never had vocoder weights: the restore entry refuses it, the validation entry ran
        with pytest.raises(RuntimeError, match="weights are not finalized"):
            eng.restore_gsr_varlen(wav, BATCH)
        # the log-mel is the restore entry's, bit for bit
        _, logmel0 = full.restore_gsr_varlen(wav, BATCH, want_logmel=True)
        assert torch.equal(logmel, logmel0.cpu())
        # val_l against the float64 host sum of |float32(lg - tlog)|, tlog = vfx_stft_mel(log10_mel = 1) of the target alone
        for b, (n, m) in enumerate(zip(BATCH, BATCH_T)):
            Tb = n // HOP + 1
            tlog = eng.stft(tgt[b:b + 1, :m], want_mel=True, log10_mel=True)["mel"][0].cpu().numpy()
            assert tlog.shape == (Tb, 128)
            value, bound = ref.mean_abs_f32_diff(logmel[b, :Tb].numpy(), tlog)
            print(module, "clip", b, "device", float(val[b]), "host", value, "|difference|", abs(float(val[b]) - value), "bound", bound)
            assert value > 0 and abs(float(val[b]) - value) <= bound, (module, b, float(val[b]), value, bound)
            # ... and the clip in a batch of one, at its own row length: the same double
            own = eng.validate_gsr_varlen(wav[b:b + 1, :m], [n], tgt[b:b + 1, :m], [m]).cpu()
            assert torch.equal(own, val[b:b + 1]), (module, b)
        # target_lengths = None: the targets have the clips' lengths
        same = eng.validate_gsr_varlen(wav, BATCH, tgt).cpu()
        tl0 = eng.stft(tgt[0:1, :BATCH[0]], want_mel=True, log10_mel=True)["mel"][0].cpu().numpy()
        value, bound = ref.mean_abs_f32_diff(logmel[0, :3].numpy(), tl0)
        assert abs(float(same[0]) - value) <= bound
    finally:
        eng.select_analysis(0)
        full.select_analysis(0)


def test_validate_gsr_varlen_130_clips(engines, many):
    eng, full = engines
    lens, prs = many
    Lmax = eng.padded_frames(max(lens)) * HOP - 1
    wav, tgt = _pad([p[0] * 50.0 for p in prs], Lmax), _pad([p[1] * 50.0 for p in prs], Lmax)
    val, logmel = eng.validate_gsr_varlen(wav, lens, tgt, want_logmel=True)
    val = val.cpu()
    assert val.shape == (130,) and torch.isfinite(val).all() and (val > 0).all()
    _, logmel0 = full.restore_gsr_varlen(wav, lens, want_logmel=True)
    assert torch.equal(logmel.cpu(), logmel0.cpu())
    for b in (0, 64, 127, 128, 129):
        n = lens[b]
        own = eng.validate_gsr_varlen(wav[b:b + 1, :n], [n], tgt[b:b + 1, :n]).cpu()
        assert torch.equal(own, val[b:b + 1]), b


def test_validate_gsr_varlen_refusals(eng):
    wav, tgt, Lmax = _val_batch(eng)
    with pytest.raises(RuntimeError, match=r"clip 1 has 11 frames \(4533 samples\) but its target has 12 \(4900 samples\)"):
        eng.validate_gsr_varlen(wav, BATCH, tgt, [1100, 4900, 28300])
    with pytest.raises(RuntimeError, match="vfx_validate_gsr_varlen: clip 2 has 1024 samples"):
        eng.validate_gsr_varlen(wav, [1025, 4533, 1024], tgt)
    with pytest.raises(RuntimeError, match="the target of clip 0 has %d samples" % (Lmax + 1)):
        eng.validate_gsr_varlen(wav, [Lmax, 4533, L65], tgt, [Lmax + 1, 4600, 28300])
    from voicefixer_main_amd.engine import _ptr
    d = wav.to(eng.device)
    out = torch.full((3,), -7.0, device=eng.device, dtype=torch.float64)
    arr = (ctypes.c_int * 3)(*BATCH)
    rc = eng.lib.vfx_validate_gsr_varlen(eng.h, _ptr(d), None, 3, Lmax, arr, None, None, _ptr(out), eng._stream())
    assert rc == 1 and "target is NULL" in eng.lib.vfx_last_error().decode()
    rc = eng.lib.vfx_validate_gsr_varlen(eng.h, _ptr(d), _ptr(d), 3, Lmax, arr, None, None, None, eng._stream())
    assert rc == 1 and "val_l is NULL" in eng.lib.vfx_last_error().decode()
    # a 3-frame clip is validated (the scored restore needs 7 frames for its SSIM; nothing here does)
    assert torch.isfinite(eng.validate_gsr_varlen(wav[:1], BATCH[:1], tgt[:1], BATCH_T[:1])).all()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((3,), -7.0, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_voicefixer_validation_step_and_validate_list(eng):
    from voicefixer_main_amd.models import VoiceFixer
    model = VoiceFixer(engine=eng)
    prs = [ref.make_pair(4533, 700 + i) for i in range(3)]
    noisy = torch.stack([torch.from_numpy(p[0] * 50.0) for p in prs])
    vocals = torch.stack([torch.from_numpy(p[1] * 50.0) for p in prs])
    out = model.validation_step({"noisy": noisy[:, :, None], "vocals": vocals[:, :, None]}, 0)
    assert set(out) == {"loss"} and out["loss"].dim() == 0 and out["loss"].dtype == torch.float64 and out["loss"].is_cuda
    per, mean = model.validate_list(list(noisy), list(vocals))
    assert len(per) == 3 and float(out["loss"]) == pytest.approx(mean, rel=1e-14)
    assert torch.equal(eng.validate_gsr_varlen(noisy, [4533] * 3, vocals).cpu(), torch.tensor(per, dtype=torch.float64))
    assert float(model.validation_step({"noisy": noisy, "vocals": vocals})["loss"]) == float(out["loss"])      # (B, L) too
    # a list of unequal lengths, handed over unsorted: every file's value is its own call's
    mixed = [ref.make_pair(n, 800 + i) for i, n in enumerate([3000, L65, 1025])]
    per, mean = model.validate_list([torch.from_numpy(p[0] * 50.0) for p in mixed], [torch.from_numpy(p[1] * 50.0) for p in mixed])
    for i, p in enumerate(mixed):
        own = eng.validate_gsr_varlen(torch.from_numpy(p[0] * 50.0)[None], [len(p[0])], torch.from_numpy(p[1] * 50.0)[None])
        assert float(own[0]) == per[i], i
    assert mean == pytest.approx(sum(per) / 3.0, rel=1e-15)


def test_ssr_unet_validation(eng):
    from voicefixer_main_amd.models import GSR_UNet, SSR_UNet
    assert GSR_UNet is SSR_UNet
    model = SSR_UNet(engine=eng)
    lens = [4533, L65, 3000]
    prs = [ref.make_pair(n, 900 + i) for i, n in enumerate(lens)]
    wavs = [torch.from_numpy(p[0] * 50.0) for p in prs]
    tgts = [torch.from_numpy(p[1] * 50.0) for p in prs]
    restored = model.restore_list(wavs)
    per, mean = model.validate_list(wavs, tgts)
    per_in, _ = model.validate_list(wavs, tgts, against="input")
    for i in range(3):
        assert float(eng.spec_losses(restored[i][None], tgts[i][None])[0, 1]) == per[i], i
        assert float(eng.spec_losses(restored[i][None], wavs[i][None])[0, 1]) == per_in[i], i
    assert mean == pytest.approx(sum(per) / 3.0, rel=1e-15) and per != per_in
    # validation_step on an equal-length batch: the mean of the files' values
    noisy, vocals = torch.stack([wavs[0], wavs[0] * 0.5]), torch.stack([tgts[0], tgts[0] * 0.5])
    out = model.validation_step({"noisy": noisy[:, :, None], "vocals": vocals[:, :, None]})
    per2, mean2 = model.validate_list(list(noisy), list(vocals))
    assert out["loss"].dim() == 0 and out["loss"].dtype == torch.float64 and float(out["loss"]) == pytest.approx(mean2, rel=1e-14)
    out_in = model.validation_step({"noisy": noisy, "vocals": vocals}, against="input")
    assert float(out_in["loss"]) == pytest.approx(sum(model.validate_list(list(noisy), list(vocals), against="input")[0]) / 2.0, rel=1e-14)


def test_loss_functions_equal_the_columns(eng, pairs):
    from voicefixer_main_amd import losses
    Lmax = L65 + 300
    est, tgt = _pad([pairs[n][0] for n in BATCH], Lmax), _pad([pairs[n][1] for n in BATCH], Lmax)
    cols = eng.spec_losses(est, tgt, BATCH)
    w_wav, w_sp = losses.mix_weights()
    want = {"l1": cols[:, 0].mean(), "l1_wav": cols[:, 0].mean(), "l1_sp": cols[:, 1].mean(), "l1_log_sp": cols[:, 2].mean(),
            "l1_wav_l1_sp": (w_wav * cols[:, 0] + w_sp * cols[:, 1]).mean(),
            "l1_wav_l1_log_sp": (w_wav * cols[:, 0] + w_sp * cols[:, 2]).mean()}
    for name, v in want.items():
        got = losses.get_loss_function(name, eng)(est[:, None], tgt[:, None], lengths=BATCH)
        assert got.dim() == 0 and got.dtype == torch.float64 and got.is_cuda and float(got) == float(v), name
    # the waveform L1 through k_l1_rows alone is column 0, clip by clip
    assert torch.equal(eng.l1_rows(est, tgt, BATCH), cols[:, 0])
    # "l1" of log-mel images (the mel case of val_l): the float64 host sum of the float32 differences
    rng = np.random.default_rng(9)
    a = rng.standard_normal((2, 1, 65, 128)).astype(np.float32)
    b = rng.standard_normal((2, 1, 65, 128)).astype(np.float32)
    got = losses.get_loss_function("l1", eng)(torch.from_numpy(a), torch.from_numpy(b))
    value, bound = ref.mean_abs_f32_diff(a, b)
    assert abs(float(got) - value) <= 2 * bound
    with pytest.raises(NotImplementedError, match="'sisnr'"):
        losses.get_loss_function("sisnr", eng)
