"""GPU: vfx_bsseval (bsseval.hip) against the float64 restatement (tests/bsseval_f64.py), stage by stage (vfx_op_bsseval_stage) and
as scores, per-clip independence of the batch, argument checks, and the `bsseval=` switch of AudioMetrics end to end.

The shapes are where the kernels can go wrong: flen 16, 48, 512 (one and two MFMA accumulators per correlation), n below flen, n no
multiple of 4 or 16, both sides of a slab boundary (the slab length is read from the library's constant), more than two slabs.  The
pad past every clip's length is NaN: any read of it shows in the scores.  tests/test_bsseval_host.py shows, on the reference alone,
that every case is well conditioned (cond <= 1e4, scores finite and below 100 dB, defined to 1e-10 dB between solvers).

The sums are held to the bound of a float64 sum of m terms in ANY order, |sum - exact| <= (m - 1) 2^-53 sum |terms|: derived, not
measured.  The exact side is summed in numpy.longdouble, whose own m 2^-64 sum |terms| is added to the bound.

Largest |device - float64| of the scores as measured on an MI355X: see DESIGN.md (bsseval.hip)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bsseval_f64 as ref
from voicefixer_main_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
UL = 2.0 ** -64                       # numpy.longdouble on x86: a 64-bit significand
S = _lib.BSSEVAL_SLAB
SCORE_TOL_DB = 1e-9
# || G c - d ||_inf / (flen 2^-53 (|| G ||_inf || c ||_inf + || d ||_inf)), the largest over the cases of this file and the pair S,
# of the two CPU solvers of bsseval_f64.py on their own (a, d); the device is given 8 x the larger
RESIDUAL_K_MEASURED_LU = 0.09924
RESIDUAL_K_MEASURED_LEVINSON = 0.08749
RESIDUAL_K = 8.0 * max(RESIDUAL_K_MEASURED_LU, RESIDUAL_K_MEASURED_LEVINSON)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd.engine import Engine
    return Engine("cuda:0")


def _batch(pairs, extra=0):
    """[(est, target)] float32 -> NaN-padded (B, Lmax + extra) tensors and the lengths."""
    lens = [len(t) for _, t in pairs]
    L = max(lens) + extra
    e = np.full((len(pairs), L), np.nan, np.float32)
    t = np.full((len(pairs), L), np.nan, np.float32)
    for b, (x, y) in enumerate(pairs):
        e[b, :len(x)], t[b, :len(y)] = x, y
    return torch.from_numpy(e), torch.from_numpy(t), lens


@functools.lru_cache(maxsize=None)
def _pairs(flen, makers="ABC"):
    return tuple(ref.pair(m, seed, n) for m, seed, n, f in ref.cases(S) if f == flen and m in makers)


@functools.lru_cache(maxsize=None)
def _reference(flen):
    return np.stack([ref.bsseval(e, r, flen) for e, r in _pairs(flen)])


@functools.lru_cache(maxsize=None)
def _pair_s():
    return ref.make_s()


def test_the_cases_cover_the_kernels_paths():
    ns = ref.lengths(S)
    assert S % 16 == 0 and {S - 1, S + 1, 2 * S + 3} <= set(ns) and min(ns) < 16 and any(n % 4 for n in ns) and max(ns) > 2 * S
    assert ref.FLENS == (16, 48, 512) and len(ref.cases(S)) == 90


# ---------------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("flen", ref.FLENS)
def test_scores_vs_float64_in_any_batch(eng, flen):
    """A, B and C at every length in ONE batch at Lmax = the longest: within 1e-9 dB of the restatement; the same clips one per call,
    and in another order in a batch with a larger Lmax and NaN past each clip's length: the same bits."""
    pairs = _pairs(flen)
    e, t, lens = _batch(pairs)
    got = eng.bsseval(e, t, lens, flen=flen).cpu()
    err = np.abs(got.numpy() - _reference(flen))
    print("flen %d: largest |device - float64| sdr %.3g isr %.3g sar %.3g dB" % ((flen,) + tuple(err.max(axis=0))))
    assert np.all(err <= SCORE_TOL_DB), (flen, err.max(axis=0))
    for b, n in enumerate(lens):
        own = eng.bsseval(e[b:b + 1, :n], t[b:b + 1, :n], flen=flen).cpu()
        assert torch.equal(own[0], got[b]), (flen, b, n, (own[0] - got[b]).tolist())
    idx = list(range(len(pairs)))[::-1]
    e2, t2, lens2 = _batch([pairs[i] for i in idx], extra=777)
    assert torch.equal(eng.bsseval(e2, t2, lens2, flen=flen).cpu(), got[idx])


def test_more_clips_than_one_sub_batch(eng):
    """1030 short clips are two sub-batches of the call (at most 1024 clips share a set of launches): the clips of the second one
    score what they score in a call of their own."""
    rng = np.random.default_rng(3)
    lens = [int(v) for v in rng.integers(17, 40, size=1030)]
    t = rng.standard_normal((1030, 40)).astype(np.float32)
    e = (0.5 * t + 0.3 * rng.standard_normal((1030, 40))).astype(np.float32)
    for b, n in enumerate(lens):
        e[b, n:], t[b, n:] = np.nan, np.nan
    got = eng.bsseval(torch.from_numpy(e), torch.from_numpy(t), lens, flen=16).cpu()
    assert torch.isfinite(got).all()
    for b0, b1 in ((0, 7), (1020, 1030)):
        own = eng.bsseval(torch.from_numpy(e[b0:b1]), torch.from_numpy(t[b0:b1]), lens[b0:b1], flen=16).cpu()
        assert torch.equal(own, got[b0:b1]), (b0, b1)
    want = ref.bsseval(e[1029, :lens[1029]], t[1029, :lens[1029]], 16)
    assert np.all(np.abs(got[1029].numpy() - want) <= SCORE_TOL_DB)


def test_quiet_pairs_where_the_eps_counts(eng):
    """Input A at 2^-24 of unit level, where the 2^-52 on the diagonal is 1e-4 of a[0] and leaving it off moves isr and sar by 1e-3 dB
    (tests/test_bsseval_host.py shows both on the reference): the device is held to the same 1e-9 dB."""
    for flen in sorted({f for _, _, f in ref.QUIET_CASES}):
        pairs = [ref.quiet_pair(seed, n) for seed, n, f in ref.QUIET_CASES if f == flen]
        e, t, lens = _batch(pairs)
        got = eng.bsseval(e, t, lens, flen=flen).cpu().numpy()
        want = np.stack([ref.bsseval(x, y, flen) for x, y in pairs])
        print("quiet, flen %d: largest |device - float64| %s dB" % (flen, np.abs(got - want).max(axis=0)))
        assert np.all(np.abs(got - want) <= SCORE_TOL_DB), (flen, got - want)


def test_identical_and_silent_pairs(eng):
    x = ref.make_a(700, 1)[1]
    z = np.zeros(700, np.float32)
    for flen in (48, 512):
        e, t, lens = _batch([(x, x), (z, x), (x, z)])
        got = eng.bsseval(e, t, lens, flen=flen).cpu().numpy()
        assert got[0, 0] == np.inf and got[0, 1] >= 200.0 and got[0, 2] >= 200.0, got[0]    # (ratios of rounding noise, or +inf)
        assert np.all(np.isnan(got[1:])), got[1:]


def test_speech_like_pair(eng):
    """The pair S (44100 samples, 512 taps, an ill-conditioned Gram matrix): the tolerance is measured against the reference, 10 x the
    LU-vs-Levinson spread of the restatement on this very pair, no less than 1e-9 and no more than 1e-6 dB."""
    e, r = _pair_s()
    want = ref.bsseval(e, r, 512)
    spread = float(np.max(np.abs(want - ref.bsseval(e, r, 512, ref.solve_levinson))))
    tol = min(max(10.0 * spread, 1e-9), 1e-6)
    got = eng.bsseval(torch.from_numpy(e), torch.from_numpy(r)).cpu().numpy()[0]
    print("pair S: scores %s, LU-vs-Levinson spread %.3g dB, tolerance %.3g dB, |device - float64| %s"
          % (want, spread, tol, np.abs(got - want)))
    assert np.all(np.isfinite(want)) and np.all(np.abs(got - want) <= tol), (got - want, tol)


# ---------------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("flen", ref.FLENS)
def test_lag_stage(eng, flen):
    """a and d of input A at every length: each lag within the bound of its own terms (the products of floats are exact in float64)."""
    pairs = _pairs(flen, "A")
    e, t, lens = _batch(pairs)
    got = eng.op_bsseval_stage("lags", e, t, lens, flen=flen).cpu().numpy()
    worst = 0.0
    for b, (x, y) in enumerate(pairs):
        exact, mag, cnt = ref.correlation_terms(x, y, flen)
        bound = np.maximum(cnt - 1, 0) * U * mag + cnt * UL * mag
        err = np.abs(got[b].astype(np.longdouble) - exact).astype(np.float64)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0)
        assert np.all(err <= bound), (flen, len(y), float(np.max(err - bound)))
    print("flen %d: largest lag error / bound %.3g" % (flen, worst))


@pytest.mark.parametrize("flen", ref.FLENS)
def test_filter_stage(eng, flen):
    """Not c itself: the residual of the device's c in the system of the device's own a and d."""
    pairs = _pairs(flen) + ((_pair_s(),) if flen == 512 else ())
    e, t, lens = _batch(pairs)
    ad = eng.op_bsseval_stage("lags", e, t, lens, flen=flen).cpu().numpy()
    c = eng.op_bsseval_stage("filter", e, t, lens, flen=flen).cpu().numpy()
    ratios = [ref.residual_ratio(ad[b, 0], ad[b, 1], c[b]) for b in range(len(pairs))]
    print("flen %d: largest residual ratio %.3g (allowed %.3g)" % (flen, max(ratios), RESIDUAL_K))
    assert np.all(np.isfinite(c)) and max(ratios) <= RESIDUAL_K, (flen, ratios)


def _padded(x, m):
    out = np.zeros(m, np.longdouble)
    out[:len(x)] = x
    return out


@pytest.mark.parametrize("flen", ref.FLENS)
def test_projection_stage(eng, flen):
    """P of input A against sum_k c[k] r[t - k] of the device's own c: m terms per output and the 2^-53 of each product."""
    pairs = _pairs(flen, "A")
    e, t, lens = _batch(pairs)
    c = eng.op_bsseval_stage("filter", e, t, lens, flen=flen).cpu().numpy()
    P = eng.op_bsseval_stage("projection", e, t, lens, flen=flen).cpu().numpy()
    assert P.shape == (len(pairs), max(lens) + flen - 1)
    worst = 0.0
    for b, (x, y) in enumerate(pairs):
        n, m = len(y), len(y) + flen - 1
        exact = np.convolve(c[b].astype(np.longdouble), y.astype(np.longdouble))
        mag = np.convolve(np.abs(c[b]), np.abs(y.astype(np.float64)))
        cnt = np.convolve(np.ones(flen), np.ones(n))
        bound = cnt * U * mag + (cnt + 1) * UL * mag
        err = np.abs(P[b, :m].astype(np.longdouble) - exact).astype(np.float64)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (flen, n, float(np.max(err / bound)))
        assert not np.any(P[b, m:]), (flen, n)
    print("flen %d: largest projection error / bound %.3g" % (flen, worst))


@pytest.mark.parametrize("flen", ref.FLENS)
def test_energy_stage(eng, flen):
    """The five energies of input A against the exact sums of their terms, the terms taken of the device's own P (the stage-3 run is
    the same projection code with its store enabled): m = n + flen - 1 terms each."""
    pairs = _pairs(flen, "A")
    e, t, lens = _batch(pairs)
    P = eng.op_bsseval_stage("projection", e, t, lens, flen=flen).cpu().numpy()
    got = eng.op_bsseval_stage("energies", e, t, lens, flen=flen).cpu().numpy()
    assert got.shape == (len(pairs), 5)
    worst = 0.0
    for b, (x, y) in enumerate(pairs):
        m = len(y) + flen - 1
        r, s, p = _padded(y, m), _padded(x, m), P[b, :m].astype(np.longdouble)
        for k, term in enumerate((r * r, (s - r) ** 2, (p - r) ** 2, p * p, (s - p) ** 2)):
            exact, mag = np.sum(term), float(np.sum(term))
            bound = (m - 1) * U * mag + 2 * m * UL * mag
            err = float(abs(np.longdouble(got[b, k]) - exact))
            worst = max(worst, err / bound)
            assert err <= bound, (flen, len(y), k, err / bound)
    print("flen %d: largest energy error / bound %.3g" % (flen, worst))


# ---------------------------------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_refused(eng):
    x = torch.rand(2, 800) - 0.5
    for flen in (0, 24, 528):
        with pytest.raises(RuntimeError, match=r"vfx_bsseval: a filter of %d taps is not supported .*multiple of 16 in \[16, 512\]" % flen):
            eng.bsseval(x, x, flen=flen)
    with pytest.raises(RuntimeError, match=r"clip 1 has 0 samples \(need 1 <= length <= Lmax = 800\)"):
        eng.bsseval(x, x, [300, 0])
    with pytest.raises(RuntimeError, match=r"clip 1 has 801 samples \(need 1 <= length <= Lmax = 800\)"):
        eng.bsseval(x, x, [300, 801])
    with pytest.raises(RuntimeError, match="vfx_bsseval: bad argument"):
        eng.bsseval(torch.zeros(0, 800), torch.zeros(0, 800))
    with pytest.raises(ValueError):
        eng.bsseval(x, x[:, :700])
    with pytest.raises(RuntimeError, match=r"stage 2 of this batch writes 10 doubles \(given 9\)"):
        out = torch.zeros(9, device=eng.device, dtype=torch.float64)
        xd = x.to(eng.device)
        _lib.check(_lib.load_test().vfx_op_bsseval_stage(eng.h, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(xd.data_ptr()), 2, 800,
                                                         (ctypes.c_int * 2)(800, 800), 16, 2, ctypes.c_void_p(out.data_ptr()), 9, None),
                   "vfx_op_bsseval_stage")
    # nothing is launched by a refused call: the output keeps what it held
    xd = x.to(eng.device)
    out = torch.full((2, 3), 7.0, device=eng.device, dtype=torch.float64)
    px, po, lens = ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(out.data_ptr()), (ctypes.c_int * 2)(300, 800)
    for args in ((None, px, 2, 800, lens, 512, po), (px, None, 2, 800, lens, 512, po), (px, px, 2, 800, None, 512, po),
                 (px, px, 2, 800, lens, 512, None), (px, px, 2, 800, lens, 24, po), (px, px, 2, 800, (ctypes.c_int * 2)(300, 801), 512, po)):
        assert eng.lib.vfx_bsseval(eng.h, *args, None) != 0
        assert eng.lib.vfx_last_error().decode().startswith("vfx_bsseval: ")
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[7.0] * 3] * 2
    assert torch.isfinite(eng.bsseval(x, 0.5 * x + 0.1 * torch.rand(2, 800), flen=16)).all()


# ---------------------------------------------------------------------------------------------------------------------- surface
def test_audio_metrics_with_stoi_and_bsseval(eng, tmp_path):
    from voicefixer_main_amd import handlers, metrics
    rng = np.random.default_rng(31)
    pairs = []
    for i, n in enumerate((3000, 4410, 3700)):
        clean = 0.2 * rng.standard_normal(n)
        handlers.save_wave(clean, str(tmp_path / ("clean%d.wav" % i)))
        handlers.save_wave(0.7 * clean + 0.05 * rng.standard_normal(n), str(tmp_path / ("noisy%d.wav" % i)))
        pairs.append((str(tmp_path / ("noisy%d.wav" % i)), str(tmp_path / ("clean%d.wav" % i))))
    both = metrics.AudioMetrics(44100, eng, stoi=True, bsseval=True).evaluation_list(pairs)
    plain = metrics.AudioMetrics(44100, eng).evaluation_list(pairs)
    for (est, tgt), r, r9 in zip(pairs, both, plain):
        assert list(r) == ["sisdr", "stoi"] + list(metrics.METRIC_KEYS[1:]) + ["sdr", "isr", "sar"]
        assert list(r9) == list(metrics.METRIC_KEYS) and {k: r[k] for k in r9} == r9
        x, y = handlers.load_wav(est), handlers.load_wav(tgt)
        own = eng.bsseval(torch.from_numpy(x), torch.from_numpy(y)).cpu().numpy()[0]
        assert [r[k] for k in ref.KEYS] == own.tolist()
        assert np.all(np.abs(own - ref.bsseval(x, y)) <= SCORE_TOL_DB)
