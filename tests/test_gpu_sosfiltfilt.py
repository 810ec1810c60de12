"""GPU: the device zero-phase IIR filter (Engine.sosfiltfilt, csrc/sosfilt.hip) against scipy.signal.sosfiltfilt bit for bit, and
the batch forms of the degradation simulator (simulate.lowpass_list / bandpass_list) built on it.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FS = 44100
NYQ = FS / 2
DEV = torch.device("cuda:0")
TILE = 64          # kSosTile (csrc/vfx_internal.h): samples of a clip per LDS tile, one wave-wide row

DESIGNS = {
    "butter2": signal.butter(2, 4000 / NYQ, output="sos"),                                   # 1 section
    "butter3": signal.butter(3, 4000 / NYQ, output="sos"),                                   # 2 sections, one with b2 = a2 = 0
    "cheby1_8": signal.cheby1(8, 0.1, 1000 / NYQ, output="sos"),
    "ellip10": signal.ellip(10, 0.1, 60, 2000 / NYQ, output="sos"),
    "bessel5": signal.bessel(5, 8000 / NYQ, output="sos"),
    "bp_butter5": signal.butter(5, [300 / NYQ, 3400 / NYQ], btype="band", output="sos"),    # 5 sections
    "bp_cheby1_10": signal.cheby1(10, 0.1, [300 / NYQ, 3400 / NYQ], btype="band", output="sos"),   # 10 sections
}


def _clips_per_wave(S):
    return 4 * min(16 // S, 8)      # sosfilt_clips_per_wave (csrc/sosfilt.hip)


def _signals(rng, n):
    """uniform noise in [-1, 1] and a full-scale +-1 square pattern"""
    return rng.uniform(-1, 1, n), np.where(rng.random(n) < 0.5, -1.0, 1.0)


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


@pytest.mark.parametrize("name", list(DESIGNS))
def test_equals_scipy(eng, name):
    """Lengths padlen + 1, padlen + 2, one sample either side of and at the tile length and twice it -- of the clip and of the
    extended clip the passes run over --, 3000 and 44 100; float32 and float64 input; noise and a full-scale square pattern.  (A
    length that is not greater than padlen is no input of sosfiltfilt: the tile lengths below the 10-section filter's padlen of 63
    are covered by the error test.)"""
    sos = DESIGNS[name]
    padlen = eng.sosfiltfilt_padlen(sos)
    S = sos.shape[0]
    lengths = {padlen + 1, padlen + 2, 3000, FS}
    for edge in (TILE, 2 * TILE):
        lengths.update({edge - 1, edge, edge + 1})
    for tiles in (2, 3, 4):             # the extended clip, and the skewed cascade's S - 1 extra steps, ending at a tile edge
        for d in (-1, 0, 1):
            lengths.update({tiles * TILE - 2 * padlen + d, tiles * TILE - 2 * padlen - (S - 1) + d})
    rng = np.random.default_rng(len(name) * 131 + S)
    for n in sorted(v for v in lengths if v > padlen):
        for x in _signals(rng, n):
            for dtype in (np.float32, np.float64):
                xd = x.astype(dtype)
                y = eng.sosfiltfilt(torch.from_numpy(xd).to(DEV), sos)
                want = torch.from_numpy(signal.sosfiltfilt(sos, xd).copy())
                assert y.dtype == torch.float64 and y.shape == want.shape
                assert torch.equal(y.cpu(), want), (name, n, dtype.__name__, (y.cpu() - want).abs().max())


def test_ten_second_clip(eng):
    sos = DESIGNS["cheby1_8"]
    x = np.random.default_rng(3).uniform(-1, 1, 10 * FS).astype(np.float32)
    y = eng.sosfiltfilt(torch.from_numpy(x).to(DEV), sos).cpu()
    want = torch.from_numpy(signal.sosfiltfilt(sos, x).copy())
    assert torch.equal(y, want), (y - want).abs().max()
    # any other dtype is converted to float64 first (SciPy extends an integer clip in its own dtype, where 2 x[0] - x[k] can wrap:
    # not followed); NumPy input is taken as well
    xi = (x[:5000] * 32767).astype(np.int16)
    assert torch.equal(eng.sosfiltfilt(xi, sos).cpu(), torch.from_numpy(signal.sosfiltfilt(sos, xi.astype(np.float64)).copy()))


@pytest.mark.parametrize("name", ["cheby1_8", "bp_butter5", "bp_cheby1_10", "butter2"])
def test_batch_with_lengths(eng, name):
    """16 clips of lengths padlen + 1 .. 3 x 44100, no two alike, each row padded with 7.0 past its end: every row is SciPy on that
    clip alone, its own single-clip call, and zero past its end.  Again with B no multiple of the clips per wave, and with B = 1."""
    sos = DESIGNS[name]
    padlen = eng.sosfiltfilt_padlen(sos)
    cpw = _clips_per_wave(sos.shape[0])
    rng = np.random.default_rng(7)
    pool = [padlen + 1, padlen + 2, TILE + 1 + padlen, 300, 1023, 4096, 9999, 3 * FS]
    pool += sorted({int(v) for v in rng.integers(padlen + 3, 3 * FS, 40)} - set(pool))
    for B, dtype in ((16, torch.float32), (cpw + 3, torch.float64), (1, torch.float32)):
        lengths = [int(v) for v in rng.permutation(pool[:B])]
        assert len(set(lengths)) == B
        batch = torch.full((B, max(lengths) + 5), 7.0, dtype=dtype)
        clips = []
        for i, n in enumerate(lengths):
            clips.append(torch.from_numpy(rng.uniform(-1, 1, n)).to(dtype))
            batch[i, :n] = clips[-1]
        y = eng.sosfiltfilt(batch.to(DEV), sos, lengths=lengths).cpu()
        assert y.dtype == torch.float64 and y.shape == batch.shape
        for i, n in enumerate(lengths):
            want = torch.from_numpy(signal.sosfiltfilt(sos, clips[i].numpy()).copy())
            assert torch.equal(y[i, :n], want), (B, i, n)
            assert torch.equal(y[i, :n], eng.sosfiltfilt(clips[i].to(DEV), sos).cpu()), (B, i, n)
            assert not y[i, n:].any(), (B, i, n)


def test_second_slice_of_a_call(eng):
    """130 clips of 100 .. 400 samples in one call (128 clips travel per launch pair, kSosMaxClips), a 2-section design, float32 and
    float64 rows padded with 7.0: every row is SciPy on that clip alone and zero past its end"""
    sos = DESIGNS["butter3"]
    assert sos.shape[0] == 2
    rng = np.random.default_rng(17)
    B = 130
    lengths = [int(v) for v in rng.integers(100, 401, B)]
    lengths[127], lengths[128], lengths[129] = 400, 100, 399
    for dtype in (torch.float32, torch.float64):
        batch = torch.full((B, 405), 7.0, dtype=dtype)
        clips = [torch.from_numpy(rng.uniform(-1, 1, n)).to(dtype) for n in lengths]
        for i, c in enumerate(clips):
            batch[i, :len(c)] = c
        y = eng.sosfiltfilt(batch.to(DEV), sos, lengths=lengths).cpu()
        assert y.dtype == torch.float64 and y.shape == batch.shape
        for i, n in enumerate(lengths):
            assert torch.equal(y[i, :n], torch.from_numpy(signal.sosfiltfilt(sos, clips[i].numpy()).copy())), (dtype, i, n)
            assert not y[i, n:].any(), (dtype, i, n)


def test_errors_launch_nothing(eng):
    import ctypes
    from voicefixer_main_amd import _lib
    sos = DESIGNS["cheby1_8"]
    padlen = eng.sosfiltfilt_padlen(sos)
    batch = torch.zeros((3, 500), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="greater than padlen, which is %d" % padlen):
        eng.sosfiltfilt(batch, sos, lengths=[500, padlen, 400])
    with pytest.raises(ValueError):
        eng.sosfiltfilt(batch, np.tile(sos[:1], (17, 1)))
    with pytest.raises(ValueError, match="all ones"):
        eng.sosfiltfilt(batch, sos * 2.0)
    # the C entry point itself: an error through vfx_last_error, y untouched
    dbl = ctypes.POINTER(ctypes.c_double)
    y = torch.full((3, 500), 5.0, dtype=torch.float64, device=DEV)
    sos17 = np.ascontiguousarray(np.tile(sos[:1], (17, 1)))
    zi = np.zeros((17, 2))

    def call(lengths, s, S, ldy=500):
        lens = (ctypes.c_int64 * 3)(*lengths)
        return eng.lib.vfx_sosfiltfilt(eng.h, ctypes.c_void_p(batch.data_ptr()), 0, 3, 500, lens, s.ctypes.data_as(dbl), S,
                                       zi.ctypes.data_as(dbl), padlen, ctypes.c_void_p(y.data_ptr()), ldy, None)
    assert call([500, 500, 500], sos17, 17) != 0 and b"17 sections" in eng.lib.vfx_last_error()
    assert call([500, padlen, 500], np.ascontiguousarray(sos), sos.shape[0]) != 0 and b"greater than padlen" in eng.lib.vfx_last_error()
    assert call([500, 501, 500], np.ascontiguousarray(sos), sos.shape[0]) != 0
    for ldy in (499, 0, -1):      # a row stride of y that does not hold the clips, a negative one included
        assert call([500, 500, 500], np.ascontiguousarray(sos), sos.shape[0], ldy=ldy) != 0
        assert b"the rows hold 500 and %d" % ldy in eng.lib.vfx_last_error()
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())
    with pytest.raises(RuntimeError, match="17 sections"):
        _lib.check(call([500, 500, 500], sos17, 17), "vfx_sosfiltfilt")


def test_list_functions_equal_the_reference_outputs(eng):
    """lowpass_list / bandpass_list over the case lists of tests/test_simulate.py against the reference's own outputs
    (tests/golden/simulate.npz), with that test's comparison; then exactly equal to the single-clip host functions."""
    from oracle.gen_golden import BANDPASS_CASES
    from voicefixer_main_amd import simulate
    g = np.load(os.path.join(ROOT, "tests", "golden", "simulate.npz"))
    x = g["x"]

    def close(a, b, what):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, what
        assert np.max(np.abs(a - b)) <= 1e-9 * max(1.0, np.max(np.abs(b))), (what, np.max(np.abs(a - b)))

    for name, (hc, order, typ) in {"butter": (4000, 5, "butter"), "cheby1": (1000, 8, "cheby1"), "ellip": (6000, 6, "ellip"),
                                   "bessel": (2000, 4, "bessel"), "substr_b": (3000, 5, "b"), "order_clamped": (3000, 14, "butter"),
                                   "stft": (8000, 5, "stft")}.items():
        got = simulate.lowpass_list([x.copy(), x[:1000].copy()], highcut=hc, fs=44100, order=order, _type=typ, engine=eng)
        close(got[0], g["lowpass_" + name], name)
        assert np.array_equal(got[0], simulate.lowpass(x.copy(), hc, 44100, order=order, _type=typ)), name
        assert np.array_equal(got[1], simulate.lowpass(x[:1000].copy(), hc, 44100, order=order, _type=typ)), name
    for name, (lc, hc, order, typ) in BANDPASS_CASES.items():
        got = simulate.bandpass_list([x.copy()], lc, hc, 44100, order=order, _type=typ, engine=eng)
        close(got[0], g["bandpass_" + name], "bandpass " + name)
        assert np.array_equal(got[0], simulate.bandpass(x.copy(), lc, hc, 44100, order=order, _type=typ)), name
    with pytest.raises(ValueError):
        simulate.bandpass_list([x], 300, 3000, 44100, _type="cheby2", engine=eng)
    with pytest.raises(ValueError):
        simulate.bandpass_list([x[:, None]], 300, 3000, 44100, engine=eng)


def test_list_functions_keep_the_order(eng):
    """A shuffled list of unequal lengths, float32 and float64 mixed, more clips than one device call takes: every result is
    SciPy's for that clip, in the caller's order; the module-level engine is used when none is given."""
    from voicefixer_main_amd import simulate
    rng = np.random.default_rng(11)
    lengths = [int(v) for v in rng.permutation(np.arange(200, 200 + 300) * 3)]
    clips = [rng.uniform(-1, 1, n).astype(np.float32 if i % 3 else np.float64) for i, n in enumerate(lengths)]
    simulate.set_engine(eng)
    got = simulate.lowpass_list(clips, 1000, FS, order=8, _type="cheby1")
    sos = signal.cheby1(8, 0.1, 1000 / NYQ, output="sos")
    assert len(got) == len(clips)
    for c, y in zip(clips, got):
        assert isinstance(y, np.ndarray) and y.dtype == np.float64 and np.array_equal(y, signal.sosfiltfilt(sos, c))
    got = simulate.bandpass_list(clips[:20], 300, 3400, FS, order=10, _type="cheby1", engine=eng, to_host=False)
    sos = DESIGNS["bp_cheby1_10"]
    for c, y in zip(clips, got):
        assert y.device.type == "cuda" and np.array_equal(y.cpu().numpy(), signal.sosfiltfilt(sos, c))


def test_device_results_feed_restore_list():
    """to_host=False results fed to VoiceFixer.restore_list equal the to_host=True results fed the same way (synthetic weights)."""
    from voicefixer_main_amd import simulate, synth
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_VOCODER
    from voicefixer_main_amd.models import VoiceFixer
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = Engine("cuda:0", config={"precision": 1})
    e.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
    e.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
    vf = VoiceFixer(None, channels=2, type_target="vocals", engine=e)
    clips = [synth.make_clips(1, s, seed=41 + i)[0, 0] for i, s in enumerate((0.4, 0.3))]
    host = simulate.lowpass_list(clips, 1000, FS, order=8, _type="cheby1", engine=e)
    dev = simulate.lowpass_list(clips, 1000, FS, order=8, _type="cheby1", engine=e, to_host=False)
    a = vf.restore_list([torch.from_numpy(h) for h in host])
    b = vf.restore_list(dev)
    assert len(a) == len(b) == 2 and all(torch.equal(p, q) for p, q in zip(a, b))


def test_stft_type_on_the_device(eng):
    """`_type="stft"` at 1000 Hz (2000 Hz <-> 44 100 Hz fits the resampler) on float32 clips equals simulate.stft_hard_lowpass bit
    for bit; a cut-off the resampler does not take (1234 Hz) and float64 clips go through the host function."""
    from voicefixer_main_amd import simulate
    rng = np.random.default_rng(13)
    clips = [rng.uniform(-1, 1, n).astype(np.float32) for n in (30001, 4410, 12345)]
    ratio = 1000 / int(FS / 2)
    assert eng.resample_supported(FS, int(ratio * FS)) and eng.resample_supported(int(ratio * FS), FS)
    got = simulate.lowpass_list(clips, 1000, FS, _type="stft", engine=eng)
    for c, y in zip(clips, got):
        want = simulate.stft_hard_lowpass(c, ratio)
        assert y.dtype == want.dtype == np.float32 and np.array_equal(y, want)
    dev = simulate.lowpass_list(clips, 1000, FS, _type="stft", engine=eng, to_host=False)
    assert all(d.device.type == "cuda" and np.array_equal(d.cpu().numpy(), y) for d, y in zip(dev, got))
    assert not eng.resample_supported(FS, int(1234 / int(FS / 2) * FS))
    mixed = [clips[1], clips[2].astype(np.float64)]
    for hc in (1234, 1000):
        got = simulate.lowpass_list(mixed, hc, FS, _type="stft", engine=eng)
        for c, y in zip(mixed, got):
            assert np.array_equal(y, simulate.lowpass(c, hc, FS, _type="stft"))
