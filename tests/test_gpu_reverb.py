"""GPU: the device RIR convolution (Engine.reverb_rir, csrc/reverb.hip) -- exact on integer data against np.convolve, inside the
derived error bound of its accumulation rule on real data, batch-invariant, with the reference's peak and normalisation -- and the
batch form of the degradation simulator built on it (simulate.reverb_rir_list)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T = 8192           # kReverbTile (csrc/vfx_internal.h): outputs per workgroup
KB = 1024          # kReverbTapBlock: taps per f32 fma chain; the block sums are combined in float64
NS = [1, 2, 31, 32, 33, T - 1, T, T + 1, 2 * T + 1, 3000]
MS = [1, 2, 31, 32, 33, KB - 1, KB, KB + 1, 2 * KB + 1]
F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


def _batch(clips):
    """clips of unequal lengths -> (zero-padded (B, Lmax) float32 array, lengths)"""
    lengths = [len(c) for c in clips]
    x = np.zeros((len(clips), max(lengths)), F32)
    for i, c in enumerate(clips):
        x[i, :lengths[i]] = c
    return x, lengths


def _run(eng, clips, h, normalize=False):
    """every clip against the one RIR h, as ONE call -> ([y_b cut to its length], peaks)"""
    x, lengths = _batch(clips)
    y, peaks = eng.reverb_rir(torch.from_numpy(x).to(DEV), torch.from_numpy(np.asarray(h, F32)).to(DEV), lengths=lengths,
                              normalize=normalize)
    y, peaks = y.cpu().numpy(), peaks.cpu().numpy()
    assert y.dtype == F32 and peaks.dtype == F32 and y.shape == x.shape
    for i, n in enumerate(lengths):
        assert not y[i, n:].any()
    return [y[i, :n] for i, n in enumerate(lengths)], peaks


@pytest.mark.parametrize("M", MS)
def test_exact_on_integers(eng, M):
    """x, h integers in [-8, 8]: every partial sum stays below 2049 * 64 < 2^24, so float32 is exact in any order -- y equals
    np.convolve in int64 cut to N, bit for bit, and the peak is the max |.| of the FULL integer convolution."""
    rng = np.random.default_rng(1000 + M)
    h = rng.integers(-8, 9, M)
    clips = [rng.integers(-8, 9, n) for n in NS]
    ys, peaks = _run(eng, [c.astype(F32) for c in clips], h.astype(F32))
    for c, y, pk in zip(clips, ys, peaks):
        full = np.convolve(c.astype(np.int64), h.astype(np.int64))
        assert np.array_equal(y, full[:len(c)].astype(F32)), (len(c), M, int(np.flatnonzero(y != full[:len(c)])[0]))
        assert pk == F32(np.abs(full).max()), (len(c), M, pk)


def _assert_bound(y, x, h, what):
    """|y - truth| <= (min(M, KB) + 2) 2^-24 S[n] + 2^-149 per sample: the gamma_K bound of a K-term f32 fma chain from zero, the
    float64 sum of the block sums (far below one f32 ulp) and the final rounding"""
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    truth = signal.convolve(x64, h64, method="direct")[:len(x)]
    S = signal.convolve(np.abs(x64), np.abs(h64), method="direct")[:len(x)]
    bound = (min(len(h), KB) + 2) * 2.0 ** -24 * S + 2.0 ** -149
    err = np.abs(y.astype(np.float64) - truth)
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


@pytest.mark.parametrize("positive", [False, True], ids=["noise", "all-positive"])
@pytest.mark.parametrize("M", MS)
def test_error_bound(eng, M, positive):
    """uniform noise in [-1, 1], and |.| of both (no cancellation: the worst case of an f32 chain)"""
    rng = np.random.default_rng(2000 + M)
    h = rng.uniform(-1, 1, M).astype(F32)
    clips = [rng.uniform(-1, 1, n).astype(F32) for n in NS]
    if positive:
        h, clips = np.abs(h), [np.abs(c) for c in clips]
    ys, _ = _run(eng, clips, h)
    for c, y in zip(clips, ys):
        _assert_bound(y, c, h, (len(c), M, positive))


def test_error_bound_long_rir(eng):
    """a synthetic RIR of 20 000 taps (20 tap blocks) against a 1-s clip"""
    from voicefixer_main_amd import synth
    h = synth.make_rir(5, 20000)
    assert h.dtype == F32 and h.shape == (20000,)
    x = np.random.default_rng(3).uniform(-1, 1, 44100).astype(F32)
    y, _ = eng.reverb_rir(torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV), normalize=False)
    assert y.shape == (44100,)
    _assert_bound(y.cpu().numpy(), x, h, "make_rir 20000")


def test_rows_are_independent(eng):
    """5 clips of different lengths (T and T + 1 among them), 3 RIRs of different lengths, a non-trivial index, y filled with NaN
    through the raw entry point: every row is that clip's own single call bit for bit and zero from its length up to ldy."""
    rng = np.random.default_rng(4)
    lengths = [T + 1, 700, T, 3000, 2 * T + 5]
    rir_lengths = [KB + 3, 50, 2 * KB + 1]
    index = [2, 0, 1, 2, 0]
    clips = [rng.uniform(-1, 1, n).astype(F32) for n in lengths]
    hs = [rng.uniform(-1, 1, m).astype(F32) for m in rir_lengths]
    x, _ = _batch(clips)
    r, _ = _batch(hs)
    ldy = x.shape[1] + 11
    xd, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(r).to(DEV)
    for normalize in (0, 1):
        y = torch.full((5, ldy), float("nan"), dtype=torch.float32, device=DEV)
        peaks = torch.full((5,), float("nan"), dtype=torch.float32, device=DEV)
        from voicefixer_main_amd import _lib
        _lib.check(eng.lib.vfx_reverb_rir(eng.h, ctypes.c_void_p(xd.data_ptr()), 5, x.shape[1], (ctypes.c_int64 * 5)(*lengths),
                                          ctypes.c_void_p(rd.data_ptr()), 3, r.shape[1], (ctypes.c_int64 * 3)(*rir_lengths),
                                          (ctypes.c_int * 5)(*index), normalize, ctypes.c_void_p(y.data_ptr()), ldy,
                                          ctypes.c_void_p(peaks.data_ptr()), None), "vfx_reverb_rir")
        torch.cuda.synchronize()
        y, peaks = y.cpu(), peaks.cpu()
        for b in range(5):
            own, pk = eng.reverb_rir(torch.from_numpy(clips[b]).to(DEV), torch.from_numpy(hs[index[b]]).to(DEV),
                                     normalize=bool(normalize))
            assert torch.equal(y[b, :lengths[b]], own.cpu()), (normalize, b)
            assert torch.equal(peaks[b], pk.cpu()), (normalize, b)
            assert not y[b, lengths[b]:].any(), (normalize, b)


def test_second_slice_of_a_call(eng):
    """130 clips in one call (128 clips travel per launch, kReverbMaxClips) == rows 0-127 and rows 128-129 each in a call of their
    own, y and peaks bit for bit, with the normalisation.  The index is explicit: the default b % R goes by the row in the call."""
    rng = np.random.default_rng(8)
    B = 130
    lengths = [int(n) for n in rng.integers(33, 601, B)]
    lengths[127], lengths[128], lengths[129] = 600, 33, 599
    rir_lengths = [40, 7, 33]
    index = [int(i) for i in rng.integers(0, 3, B)]
    x, _ = _batch([(rng.uniform(-1, 1, n) * (0.05, 1.0)[b % 2]).astype(F32) for b, n in enumerate(lengths)])      # either side of 0.99
    r, _ = _batch([rng.uniform(-1, 1, m).astype(F32) for m in rir_lengths])
    xd, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(r).to(DEV)

    def run(lo, hi):
        return eng.reverb_rir(xd[lo:hi], rd, rir_index=index[lo:hi], lengths=lengths[lo:hi], rir_lengths=rir_lengths, normalize=True)
    (y, peaks), (y0, peaks0), (y1, peaks1) = run(0, B), run(0, 128), run(128, B)
    assert y.shape == (B, 600) and torch.equal(y, torch.cat([y0, y1])) and torch.equal(peaks, torch.cat([peaks0, peaks1]))
    scaled = peaks > 0.99
    assert bool(scaled.any()) and not bool(scaled.all()) and bool((peaks > 0).all())
    for b in (0, 127, 128, 129):      # and the rows are what the clip alone gives
        own, pk = eng.reverb_rir(xd[b, :lengths[b]], rd[index[b], :rir_lengths[index[b]]], normalize=True)
        assert torch.equal(y[b, :lengths[b]], own) and torch.equal(peaks[b], pk) and not bool(y[b, lengths[b]:].any())


def test_peak_covers_the_tail(eng):
    """x = e_99 of 100 samples, h = 0.5 at tap 0 and 2.0 at tap 49: the written samples peak at 0.5, the full convolution at 2.0"""
    x = np.zeros(100, F32)
    x[99] = 1.0
    h = np.zeros(50, F32)
    h[0], h[49] = 0.5, 2.0
    y, peak = eng.reverb_rir(torch.from_numpy(x).to(DEV), torch.from_numpy(h).to(DEV))
    y, peak = y.cpu().numpy(), peak.cpu().numpy()
    assert peak == F32(2.0)
    want = F32(F32(0.5) / F32(2.0)) * F32(0.98)
    assert y.dtype == F32 and y[99] == want and not y[:99].any()


def test_normalisation_is_numpys(eng):
    """noise clips scaled so that the full convolution peaks at 0.6 or at 1.7 in turn: a row with (double)peak > 0.99 equals
    (raw / float32(peak)) * float32(0.98) evaluated in float32, every other row equals raw, bit for bit"""
    rng = np.random.default_rng(6)
    h = rng.uniform(-1, 1, KB + 1).astype(F32)
    clips = []
    for i, n in enumerate(NS):
        c = rng.uniform(-1, 1, n)
        c *= (0.6, 1.7)[i % 2] / np.abs(np.convolve(c, h.astype(np.float64))).max()
        clips.append(c.astype(F32))
    raw, peaks = _run(eng, clips, h, normalize=False)
    got, peaks_n = _run(eng, clips, h, normalize=True)
    assert np.array_equal(peaks, peaks_n)
    scaled = [float(p) > 0.99 for p in peaks]
    assert any(scaled) and not all(scaled)
    for r, g, p, s in zip(raw, got, peaks, scaled):
        want = (r / F32(p)) * F32(0.98) if s else r
        assert want.dtype == F32 and np.array_equal(g, want), (len(r), p)


def test_reverb_rir_list(eng):
    """mixed lengths, float32 and float64 clips mixed, a shuffled index: results in the caller's order; a float64 clip equals the host
    function exactly, a float32 clip equals Engine.reverb_rir of the clip alone bit for bit; device results stay on the device"""
    from voicefixer_main_amd import simulate, synth
    rng = np.random.default_rng(7)
    lengths = [5000, 300, T + 1, 1200, 9000, 33, 2500]
    rirs = [synth.make_rir(1, 1500), synth.make_rir(2, 400).astype(np.float64), synth.make_rir(3, 2 * KB + 1)]
    index = [2, 0, 1, 0, 2, 0, 1]
    clips = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float64 if i == 3 else F32) for i, n in enumerate(lengths)]
    got = simulate.reverb_rir_list(clips, rirs, rir_index=index, engine=eng)
    dev = simulate.reverb_rir_list(clips, rirs, rir_index=index, engine=eng, to_host=False)
    assert len(got) == len(dev) == len(clips)
    for c, i, y, d in zip(clips, index, got, dev):
        assert isinstance(y, np.ndarray) and d.device.type == "cuda" and np.array_equal(d.cpu().numpy(), y)
        if c.dtype == F32 and rirs[i].dtype == F32:
            own, _ = eng.reverb_rir(torch.from_numpy(c).to(DEV), torch.from_numpy(rirs[i]).to(DEV))
            assert y.dtype == F32 and np.array_equal(y, own.cpu().numpy())
        else:
            assert np.array_equal(y, simulate.reverb_rir(c, rirs[i]))
    one = simulate.reverb_rir_list(clips[:2], rirs[0], engine=eng)      # one RIR for every clip
    assert np.array_equal(one[1], eng.reverb_rir(clips[1], rirs[0])[0].cpu().numpy())
    with pytest.raises(ValueError):
        simulate.reverb_rir_list(clips, rirs, rir_index=[3] * len(clips), engine=eng)


def test_device_results_feed_restore_list(engine):
    """a to_host=False result fed to VoiceFixer.restore_list equals the to_host=True result fed the same way"""
    from voicefixer_main_amd import simulate, synth
    from voicefixer_main_amd.models import VoiceFixer
    vf = VoiceFixer(None, channels=2, type_target="vocals", engine=engine)
    clips = [synth.make_clips(1, 0.3, seed=43)[0, 0]]
    rir = synth.make_rir(9, 3000)
    host = simulate.reverb_rir_list(clips, rir, engine=engine)
    dev = simulate.reverb_rir_list(clips, rir, engine=engine, to_host=False)
    a = vf.restore_list([torch.from_numpy(h) for h in host])
    b = vf.restore_list(dev)
    assert len(a) == len(b) == 1 and torch.equal(a[0], b[0])


def test_errors_launch_nothing(eng):
    """an empty clip, an empty RIR, an index out of range, ldy too small: the library's text, y and peaks untouched"""
    x = torch.zeros((3, 500), dtype=torch.float32, device=DEV)
    r = torch.ones((2, 40), dtype=torch.float32, device=DEV)
    y = torch.full((3, 500), 5.0, dtype=torch.float32, device=DEV)
    peaks = torch.full((3,), 5.0, dtype=torch.float32, device=DEV)

    def call(lengths, rir_lengths, index, ldy=500, peaks_ptr=True, normalize=1):
        return eng.lib.vfx_reverb_rir(eng.h, ctypes.c_void_p(x.data_ptr()), 3, 500, (ctypes.c_int64 * 3)(*lengths),
                                      ctypes.c_void_p(r.data_ptr()), 2, 40, (ctypes.c_int64 * 2)(*rir_lengths), (ctypes.c_int * 3)(*index),
                                      normalize, ctypes.c_void_p(y.data_ptr()), ldy,
                                      ctypes.c_void_p(peaks.data_ptr()) if peaks_ptr else None, None)
    assert call([500, 0, 500], [40, 40], [0, 1, 0]) != 0 and b"clip 1 is empty" in eng.lib.vfx_last_error()
    assert call([500, 500, 500], [40, 0], [0, 1, 0]) != 0 and b"RIR 1 is empty" in eng.lib.vfx_last_error()
    assert call([500, 500, 500], [40, 40], [0, 2, 0]) != 0 and b"asks for RIR 2 of 2" in eng.lib.vfx_last_error()
    assert call([500, 500, 500], [40, 40], [0, -1, 0]) != 0
    assert call([500, 500, 500], [40, 40], [0, 1, 0], ldy=499) != 0 and b"too small" in eng.lib.vfx_last_error()
    assert call([500, 500, 500], [40, 41], [0, 1, 0]) != 0
    assert call([500, 501, 500], [40, 40], [0, 1, 0]) != 0
    assert call([500, 500, 500], [40, 40], [0, 1, 0], peaks_ptr=False) != 0 and b"peaks" in eng.lib.vfx_last_error()
    torch.cuda.synchronize()
    assert bool((y == 5.0).all()) and bool((peaks == 5.0).all())
    with pytest.raises(RuntimeError, match="clip 1 is empty"):
        eng.reverb_rir(x, r, lengths=[500, 0, 500])
    with pytest.raises(RuntimeError, match="RIR 0 is empty"):
        eng.reverb_rir(x, r, rir_lengths=[0, 40])
    with pytest.raises(RuntimeError, match="asks for RIR 5"):
        eng.reverb_rir(x, r, rir_index=[0, 5, 1])
    assert call([500, 500, 500], [40, 40], [0, 1, 0], peaks_ptr=False, normalize=0) == 0     # peaks may be NULL without normalize
    torch.cuda.synchronize()
    assert bool((y[:, :39] == 0.0).all())
