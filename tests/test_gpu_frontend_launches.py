"""GPU: the STFT / ISTFT front end (csrc/stft.hip) and the glue launches between the models of a restore call (csrc/small_ops.hip), one
launcher at a time through libvfx_test.so (vfx_op_stft, vfx_op_istft, vfx_op_from_log, vfx_op_voc_prep, vfx_op_peak_trim and the peak of
vfx_op_voc_final), against the float64 forms of tests/frontend_f64.py -- the third part of the launch-level series beside
test_gpu_vocoder_launches.py and test_gpu_resunet_launches.py.

Every output starts as NaN and must come back finite; in the varlen cases the padding of the INPUTS is NaN too (samples at and past a
clip's length, spectrum rows at and past its frame count): neither kernel may read it.  The forward cases walk the frames-per-wave
geometries F = 1, 2, 3, 8 and the cap of 32, the inverse cases both group sizes IH = 2 and 16; each asserts the geometry it claims
through the launchers' own host-side functions.  A clip of a batch must be bit for bit what a launch of that clip alone gives (F = 1,
IH = 2, no lengths): the per-frame arithmetic depends on neither."""
import numpy as np
import pytest
import torch

import frontend_f64 as R
from voicefixer_main_amd import _lib, synth
from voicefixer_main_amd.engine import Engine, MODEL_VOCODER

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    """One handle in the default arithmetic mode with the vocoder finalized: none of these launches depends on the mode."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine("cuda:0")
    e.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
    return e


@pytest.fixture(scope="module")
def clips65():
    """1024 clips of 28241 samples (65 frames), float32 (1024, 28241): shared, never written"""
    x = synth.make_clips(1024, R.L65 / 44100.0)[:, 0]
    assert x.shape == (1024, R.L65) and x.dtype == np.float32
    return x


@pytest.fixture(scope="module")
def mel65(clips65):
    """The float64 mel of every clip of clips65, built in chunks of 64 clips, once"""
    return R.stft_ref_chunked(clips65, want=("mel",))["mel"]


def _pad_nan(clips):
    """list of (n_b,) float32 -> (B, max n) float32, NaN at and past each clip's length"""
    out = np.full((len(clips), max(c.shape[0] for c in clips)), NAN, np.float32)
    for b, c in enumerate(clips):
        out[b, :c.shape[0]] = c
    return out


def _short_clips(lengths, source=None):
    """Clips of the given lengths: the heads of synth.make_clips rows (of `source` where given)"""
    if source is None:
        source = synth.make_clips(len(lengths), max(lengths) / 44100.0)[:, 0]
    assert source.shape[0] >= len(lengths) and source.shape[1] >= max(lengths)
    return [np.ascontiguousarray(source[b, :n]) for b, n in enumerate(lengths)]


# ---------------------------------------------------------------------------------------------------------------------------------
# forward STFT
# ---------------------------------------------------------------------------------------------------------------------------------
def _finite(out, what):
    for k, v in out.items():
        assert torch.isfinite(v).all(), (what, k, "NaN left or produced")


def _assert_clip_f64(got, ref, what):
    """One clip's outputs (float32 numpy, (T_b, .)) against float64 at the bounds of test_gpu_kernels.py::test_stft_mag_phase_mel,
    relative to the clip's own largest magnitude / mel value."""
    fig = {}
    if "sp" in got:
        scale = ref["sp"].max()
        sp = got["sp"].astype(np.float64)
        fig["sp"] = np.abs(sp - ref["sp"]).max() / scale
        if "cos" in got:      # the phase through re / im, so that near-zero bins do not dominate
            fig["re"] = np.abs(sp * got["cos"] - ref["re"]).max() / scale
            fig["im"] = np.abs(sp * got["sin"] - ref["im"]).max() / scale
    if "mel" in got:
        fig["mel"] = np.abs(got["mel"].astype(np.float64) - ref["mel"]).max() / ref["mel"].max()
    bound = {"sp": 2e-6, "re": 3e-6, "im": 3e-6, "mel": 1e-5}
    for k, v in fig.items():
        assert v < bound[k], (what, k, "max |got - ref| / max ref = %.3g, bound %.3g" % (v, bound[k]))
    return fig


def _assert_logmel_f64(got, ref_mel, what):
    d = np.abs(got.astype(np.float64) - R.to_log(ref_mel))
    assert d.max() < 1e-3 and d.mean() < 1e-5, (what, "log-mel: max %.3g (bound 1e-3), mean %.3g (bound 1e-5)" % (d.max(), d.mean()))
    return d.max(), d.mean()


def _worst(figs):
    return {k: "%.3g" % max(f[k] for f in figs if k in f) for k in sorted(set().union(*figs))}


def _alone(eng, clip, want, eps=1e-8, log10_mel=False):
    """The clip in a launch of its own: B = 1, F = 1, no lengths -> dict of device tensors (1, T_b, .)"""
    assert Engine.plan_stft_frames_per_group(R.frames(clip.shape[0])) == 1
    out = eng.op_stft(clip[None], want=want, eps=eps, log10_mel=log10_mel)
    _finite(out, "alone")
    return out


def _assert_bit_identical(eng, out, clips, which, want, what, **kw):
    for b in which:
        Tb = R.frames(clips[b].shape[0])
        one = _alone(eng, clips[b], want, **kw)
        for k in want:
            assert one[k].shape[1] == Tb
            assert torch.equal(out[k][b, :Tb], one[k][0]), (what, b, k, "differs from the launch of the clip alone by %.3g" %
                                                            (out[k][b, :Tb] - one[k][0]).abs().max().item())


def _cpu(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


ALL4 = ("mel", "sp", "cos", "sin")


def test_stft_edge_lengths(eng):
    """F = 1, lengths from the shortest the reflection allows (1025: every frame reflects at both ends) to 11 frames: all four outputs
    at eps = 1e-8, mel + sp at eps = 0 (the form vfx_audio_metrics launches), the log-mel form; rows past a clip's frames exactly 0 (-8)."""
    lens = R.EDGE_LENGTHS
    B, L = len(lens), max(lens)
    T = R.frames(L)
    assert Engine.plan_stft_frames_per_group(B * T) == 1
    clips = _short_clips(lens)
    wav = _pad_nan(clips)
    refs = {}
    for eps, want in ((1e-8, ALL4), (0.0, ("mel", "sp"))):
        out = eng.op_stft(wav, T=T, lens=lens, eps=eps, want=want)
        _finite(out, ("edges", eps))
        _assert_bit_identical(eng, out, clips, range(B), want, ("edges", eps), eps=eps)
        got = _cpu(out)
        ref = refs[eps] = R.stft_ref_varlen(clips, T, eps=eps, want=("sp", "re", "im", "mel") if "cos" in want else ("sp", "mel"))
        figs = []
        for b, n in enumerate(lens):
            Tb = R.frames(n)
            figs.append(_assert_clip_f64({k: got[k][b, :Tb] for k in want}, {k: v[b, :Tb] for k, v in ref.items()}, ("edges", eps, b, n)))
            for k in want:
                assert not got[k][b, Tb:].any(), ("edges", eps, b, k, "rows past the clip's frames are not zero")
        print("edges eps=%g: worst relative figures %s" % (eps, _worst(figs)))
    lg = eng.op_stft(wav, T=T, lens=lens, log10_mel=True, want=("mel",))
    _finite(lg, "edges log-mel")
    _assert_bit_identical(eng, lg, clips, range(B), ("mel",), "edges log-mel", log10_mel=True)
    lg = lg["mel"].cpu().numpy()
    for b, n in enumerate(lens):
        Tb = R.frames(n)
        mx, mean = _assert_logmel_f64(lg[b, :Tb], refs[1e-8]["mel"][b, :Tb], ("edges", b, n))
        print("edges log-mel clip %d (%d samples): max %.3g mean %.3g" % (b, n, mx, mean))
        assert (lg[b, Tb:] == -8.0).all(), ("edges log-mel", b, "rows past the clip's frames are not -8")


def test_stft_two_frames_per_wave(eng, clips65, mel65):
    """F = 2 over 65 frames: 33 groups per clip, the last one of a single frame (no prefetch behind it)."""
    B, T = 48, 65
    assert Engine.plan_stft_frames_per_group(B * T) == 2 and -(-T // 2) == 33 and T % 2 == 1
    clips = list(clips65[:B])
    out = eng.op_stft(clips65[:B], want=ALL4)
    _finite(out, "F=2")
    _assert_bit_identical(eng, out, clips, range(B), ALL4, "F=2")
    got = _cpu(out)
    ref = R.stft_ref(clips65[:B])
    assert np.allclose(ref["mel"], mel65[:B], rtol=1e-12, atol=0)
    figs = [_assert_clip_f64({k: got[k][b] for k in ALL4}, {k: v[b] for k, v in ref.items()}, ("F=2", b)) for b in range(B)]
    print("F=2: worst relative figures %s" % _worst(figs))


def test_stft_three_frames_per_wave_varlen(eng, clips65):
    """F = 3 with per-clip lengths: last groups of three, two and one frame, groups wholly past a clip's end (the 1025-sample clip has 3
    of its row's 65 frames), the reflection at each clip's own end while the NEXT samples of its row are NaN."""
    lens = R.f3_lengths()
    B, T = len(lens), R.frames(max(lens))
    assert (B, T) == (80, 65) and Engine.plan_stft_frames_per_group(B * T) == 3
    clips = _short_clips(lens, clips65)
    out = eng.op_stft(_pad_nan(clips), T=T, lens=lens, want=ALL4)
    _finite(out, "F=3")
    _assert_bit_identical(eng, out, clips, range(B), ALL4, "F=3")
    got = _cpu(out)
    figs = []
    for b, n in enumerate(lens):
        Tb = R.frames(n)
        ref = R.stft_ref(clips[b][None])
        figs.append(_assert_clip_f64({k: got[k][b, :Tb] for k in ALL4}, {k: v[0] for k, v in ref.items()}, ("F=3", b, n)))
        for k in ALL4:
            assert not got[k][b, Tb:].any(), ("F=3", b, k, "rows past the clip's frames are not zero")
    print("F=3 varlen: worst relative figures %s" % _worst(figs))


@pytest.mark.parametrize("B,F", [(225, 8), (1024, 32)], ids=["F8-benched", "F32-cap"])
def test_stft_mel_only_long_walks(eng, clips65, mel65, B, F):
    """The mel-only kernel of the restore path (k_stft_mel<false>) at the benched launch's F = 8 and at the cap of 32 frames per wave
    (66560 frames would ask for 33): float64 for every clip, bit-identity for 16 of them, the first and the last included."""
    T = 65
    assert Engine.plan_stft_frames_per_group(B * T) == F
    assert F == 8 or -(-B * T // 2048) > 32
    out = eng.op_stft(clips65[:B], want=("mel",))
    _finite(out, ("mel-only", F))
    which = sorted(set(np.linspace(0, B - 1, 16).astype(int).tolist()))
    assert len(which) == 16 and which[0] == 0 and which[-1] == B - 1
    _assert_bit_identical(eng, out, list(clips65[:B]), which, ("mel",), ("mel-only", F))
    got = out["mel"].cpu().numpy().astype(np.float64)
    ref = mel65[:B]
    rel = np.abs(got - ref).max(axis=(1, 2)) / ref.max(axis=(1, 2))
    print("mel-only F=%d: worst max |got - ref| / max ref over %d clips = %.3g" % (F, B, rel.max()))
    assert rel.max() < 1e-5, (F, int(rel.argmax()), rel.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# ISTFT
# ---------------------------------------------------------------------------------------------------------------------------------
def _istft_varlen_case(eng, lens, IH, what):
    B, L = len(lens), max(lens)
    T = R.frames(L)
    assert Engine.plan_istft_grid(B, T, L)[0] == IH
    clips = _short_clips(lens)
    re = np.full((B, T, R.NBINS), NAN, np.float32)      # rows at and past a clip's frames stay NaN: they do not exist for it
    im = np.full((B, T, R.NBINS), NAN, np.float32)
    for b, c in enumerate(clips):
        re[b, :R.frames(lens[b])], im[b, :R.frames(lens[b])] = R.spectrum32(c)
    got = eng.op_istft(re, im, L, lens=lens)
    assert torch.isfinite(got).all(), (what, "NaN left or read")
    worst = 0.0
    for b, n in enumerate(lens):
        Tb = R.frames(n)
        assert Engine.plan_istft_grid(1, Tb, n)[0] == 2
        one = eng.istft(torch.from_numpy(re[b:b + 1, :Tb]), torch.from_numpy(im[b:b + 1, :Tb]), n)      # vfx_istft of the clip alone
        assert torch.equal(got[b, :n], one[0]), (what, b, n, "differs from the clip alone by %.3g" % (got[b, :n] - one[0]).abs().max().item())
        assert not got[b, n:].any(), (what, b, n, "samples past the clip's length are not zero")
        ref = R.istft_ref(re[b:b + 1, :Tb], im[b:b + 1, :Tb], n)[0]
        err = np.abs(got[b, :n].cpu().numpy() - ref).max()
        worst = max(worst, err)
        assert err < 5e-6, (what, b, n, err)
    print("%s: worst max |got - ref| = %.3g" % (what, worst))


def test_istft_edge_lengths_varlen(eng):
    _istft_varlen_case(eng, R.EDGE_LENGTHS, 2, "istft IH=2 varlen")


def test_istft_large_batch_varlen(eng):
    lens = R.large_istft_lengths()
    assert len(lens) == 128 and R.frames(max(lens)) == 33
    _istft_varlen_case(eng, lens, 16, "istft IH=16 varlen")


def test_istft_large_batch_frames_short_of_the_length(eng):
    """IH = 16 without lengths, 64 frames for rows of 80 hops: the overlap-add buffer ends inside the row -- zeros past it, and the
    division by the vanishing envelope of its last window as test_gpu_kernels.py::test_istft_roundtrip_and_oracle splits it."""
    from oracle import dsp
    B, T, L = 64, 64, R.HOP * 80
    assert Engine.plan_istft_grid(B, T, L) == (16, 6) and Engine.plan_istft_grid(1, T, L)[0] == 2
    wav = synth.make_clips(B, L / 44100.0)[:, 0]
    assert wav.shape == (B, L)
    re, im = dsp.stft(wav.astype(np.float64))
    re, im = np.ascontiguousarray(re[:, :T]).astype(np.float32), np.ascontiguousarray(im[:, :T]).astype(np.float32)
    got = eng.op_istft(re, im, L)
    assert torch.isfinite(got).all()
    for b in range(B):
        one = eng.istft(torch.from_numpy(re[b:b + 1]), torch.from_numpy(im[b:b + 1]), L)
        assert torch.equal(got[b], one[0]), (b, "differs from the clip alone by %.3g" % (got[b] - one[0]).abs().max().item())
    got = got.cpu().numpy()
    end = 1024 + R.HOP * (T - 1)
    assert not got[:, end:].any()
    ref = R.istft_ref(re, im, L)
    well = end - 300       # up to 300 samples before the end of the last window, w^2 >= 0.04; past that the division by the
    e0 = np.abs(got[:, :well] - ref[:, :well]).max()       # vanishing envelope amplifies fp32 rounding
    e1 = np.abs(got[:, well:] - ref[:, well:]).max()
    print("istft IH=16, 64 of 81 frames: max |got - ref| = %.3g before the last 300 samples of the buffer, %.3g in them" % (e0, e1))
    assert e0 < 5e-6
    assert e1 < 0.05 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------------------------------
# glue
# ---------------------------------------------------------------------------------------------------------------------------------
def _margined(measured, cap):
    """The bound for an error that cannot be derived here: four times the measured maximum, rounded up to a power of two -- the margin
    for other inputs and seeds -- and at most `cap` (a condition, not a measurement: the defects the case is there for lie far above it)."""
    return min(cap, 2.0 ** np.ceil(np.log2(4.0 * measured)))


# exp10f on this runtime: max |got / ref - 1| over from_log_inputs() measured on an MI355X (ROCm 7): 7.72e-08 -> the bound is 2^-21
FROM_LOG_MEASURED = 7.72e-8
FROM_LOG_BOUND = _margined(FROM_LOG_MEASURED, 1e-5)
assert FROM_LOG_BOUND == 2.0 ** -21
# k_voc_prep (log10f and the affine map in fp32): max |got - ref| over voc_prep_inputs(2, 65) and (2, 66) measured on an MI355X:
# 1.20e-06 (9.89e-07 with lengths) -> the bound is 2^-17
VOC_PREP_MEASURED = 1.20e-6
VOC_PREP_BOUND = _margined(VOC_PREP_MEASURED, 1e-4)
assert VOC_PREP_BOUND == 2.0 ** -17


def test_from_log(eng):
    """10 ** min(x, 5) over [-9, 6.5] with 5.0 itself and its neighbours; T = 65 is odd, so 256-thread blocks straddle the clips."""
    x = R.from_log_inputs(3, 65)
    got = eng.op_from_log(x)
    assert torch.isfinite(got).all()
    got = got.cpu().numpy()
    ref = R.from_log(x)
    rel = np.abs(got / ref - 1.0)
    print("from_log: max |got / ref - 1| = %.3g (bound %.3g)" % (rel.max(), FROM_LOG_BOUND))
    assert rel.max() <= FROM_LOG_BOUND, (rel.max(), x.reshape(-1)[rel.argmax()])


@pytest.mark.parametrize("lens_t", [None, [65, 1, 37]], ids=["all-frames", "lens"])
def test_from_log_unify_energy(eng, lens_t):
    """The energy match of unify_energy: every element is the launch's own unify = 0 value times sum(mel_in) / sum(estimate) over the bins
    5..24 and the clip's frames.  The sums' terms are positive, so whatever order the float atomics add them in, each sum is within
    (n - 1) roundings of the float64 sum, n = 20 * frames: |got / ref - 1| <= (2 n + 2) * 2^-24.  The bins 4 and 25 and the frames past a
    clip's end hold values that throw the ratio far outside that if they are taken in (tests/test_frontend_f64_host.py)."""
    B, T = 3, 65
    lg, tgt = R.unify_inputs(B, T, lens_t)
    est = eng.op_from_log(lg).cpu().numpy()
    got = eng.op_from_log(lg, tgt, unify=True, lens_t=lens_t)
    assert torch.isfinite(got).all()
    got = got.cpu().numpy().astype(np.float64)
    ratio = R.unify_ratio(est, tgt, lens_t)
    for b in range(B):
        n = T if lens_t is None else lens_t[b]
        rel = np.abs(got[b] / (est[b].astype(np.float64) * ratio[b]) - 1.0).max()
        print("unify clip %d (%d frames): max |got / ref - 1| = %.3g, bound %.3g" % (b, n, rel, R.unify_bound(n)))
        assert rel <= R.unify_bound(n), (b, n, rel, R.unify_bound(n))


@pytest.mark.parametrize("T", [65, 66])
@pytest.mark.parametrize("with_lens", [False, True], ids=["all-frames", "lens"])
def test_voc_prep(eng, T, with_lens):
    """The vocoder's input normalisation on zeros, negative values, values under amp_floor and values that clip at +R; Tp = T + T % 2 + 4
    rows per clip, those at and past a clip's frames exactly -R."""
    B, Tp = 2, R.voc_tp(T)
    lens_t = [T, 9] if with_lens else None
    x = R.voc_prep_inputs(B, T)
    if with_lens:
        x[1, 9:] = NAN                      # frames the clip does not have: never read
    got = eng.op_voc_prep(x, Tp, lens_t)
    assert got.shape == (B, Tp, 128) and torch.isfinite(got).all()
    got = got.cpu().numpy()
    ref = R.voc_prep_ref(np.nan_to_num(x), Tp, lens_t)
    Rg = float(eng.cfg.voc_norm_range)
    for b in range(B):
        n = T if lens_t is None else lens_t[b]
        assert (got[b, n:] == -Rg).all(), (b, "rows at and past the clip's frames are not -R")
    assert (got[:, 3] == Rg).all() and (got[0, 1] == -Rg).all()
    err = np.abs(got - ref).max()
    print("voc_prep T=%d lens=%s: max |got - ref| = %.3g (bound %.3g)" % (T, lens_t, err, VOC_PREP_BOUND))
    assert err <= VOC_PREP_BOUND


def _ulp32(ref):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("L", [28241, 28240])
def test_peak_trim(eng, L):
    """The fixed form: the centre L of 70 * 441 samples (an odd and an even difference).  A clip whose peak does not exceed 1 -- 1.0
    itself included -- is copied bit for bit, one above it divided within 1 ulp, and only that raises VFX_FLAG_PEAK_NORMALISED."""
    Llong = 70 * R.HOP
    x = np.random.default_rng(51).uniform(-1.75, 1.75, size=(3, Llong)).astype(np.float32)
    off = (Llong - L) // 2
    eng.take_flags()
    peaks = [0.5, 1.0, 1.75]
    got = eng.op_peak_trim(x, L, peaks)
    assert torch.isfinite(got).all()
    got = got.cpu().numpy()
    ref, divided = R.peak_trim_ref(x, L, peaks)
    assert divided.tolist() == [False, False, True]
    assert np.array_equal(got[0], x[0, off:off + L]) and np.array_equal(got[1], x[1, off:off + L])
    assert (np.abs(got[2] - ref[2]) <= _ulp32(ref[2])).all()
    assert np.abs(got[2] - x[2, off:off + L]).max() > 0.1
    assert eng.take_flags() & _lib.FLAG_PEAK_NORMALISED
    got = eng.op_peak_trim(x, L, [0.5, 1.0, 0.999]).cpu().numpy()
    assert np.array_equal(got, x[:, off:off + L])
    assert eng.take_flags() == 0


def test_peak_trim_varlen(eng):
    """The varlen form: clip b is the centre lens_l[b] of ITS lens_tp[b] * 441 vocoder samples (what lies behind them in its row is NaN
    here), zeros behind it in the output."""
    Llong, L = 70 * R.HOP, 28241
    lens_l = [28241, 12345, 1025]
    lens_tp = [R.voc_tp(R.frames(n)) for n in lens_l]
    x = np.random.default_rng(52).uniform(-1.75, 1.75, size=(3, Llong)).astype(np.float32)
    for b in range(3):
        x[b, lens_tp[b] * R.HOP:] = NAN
    peaks = [0.5, 2.0, 1.0]
    eng.take_flags()
    got = eng.op_peak_trim(x, L, peaks, lens_l, lens_tp)
    assert torch.isfinite(got).all()
    got = got.cpu().numpy()
    ref, divided = R.peak_trim_ref(x, L, peaks, lens_l, lens_tp)
    assert divided.tolist() == [False, True, False]
    for b, n in enumerate(lens_l):
        off = (lens_tp[b] * R.HOP - n) // 2
        if divided[b]:
            assert (np.abs(got[b, :n] - ref[b, :n]) <= _ulp32(ref[b, :n])).all()
        else:
            assert np.array_equal(got[b, :n], x[b, off:off + n])
        assert not got[b, n:].any(), (b, "samples past the clip's length are not zero")
    assert eng.take_flags() & _lib.FLAG_PEAK_NORMALISED
    got = eng.op_peak_trim(x, L, [1.0, 0.25, 1.0], lens_l, lens_tp).cpu().numpy()      # no peak above 1: copies, and no flag
    for b, n in enumerate(lens_l):
        off = (lens_tp[b] * R.HOP - n) // 2
        assert np.array_equal(got[b, :n], x[b, off:off + n]) and not got[b, n:].any()
    assert eng.take_flags() == 0


@pytest.mark.parametrize("x_f16", [False, True], ids=["f32-trunk", "f16-trunk"])
@pytest.mark.parametrize("C", [32, 64, 128])
def test_voc_final_peak(eng, C, x_f16):
    """The per-clip peak the vocoder tail hands the peak normalisation: max |wav[b, :len_b]| of the launch's own output, bit for bit, in
    every kernel form of the tail; T = 700 spans several workgroups, and with lengths a clip's peak stops at its own end."""
    B, T = 3, 700
    g = torch.Generator().manual_seed(900 + C + int(x_f16))
    x = torch.randn((B, T, C), generator=g)
    w = torch.randn((1, C, 7), generator=g) * (2.0 / np.sqrt(7 * C))
    for lens in (None, [700, 333, 5]):
        wav, peak = eng.op_voc_final(x, w.numpy(), 0.05, 0.2, x_f16=x_f16, lens=lens, want_peak=True)
        assert torch.isfinite(peak).all()
        for b in range(B):
            n = T if lens is None else lens[b]
            assert torch.isfinite(wav[b, :n]).all() and torch.isnan(wav[b, n:]).all()
            assert torch.equal(peak[b], wav[b, :n].abs().max()), (C, x_f16, lens, b, peak[b].item(), wav[b, :n].abs().max().item())
        # the clips differ: a peak taken over another clip's samples, or past a clip's end, would show
        assert len(set(peak.tolist())) == B
