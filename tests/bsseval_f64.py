"""BSS Eval v4 "images" SDR, ISR and SAR (Vincent, Gribonval, Fevotte, "Performance measurement in blind audio source separation",
IEEE TASLP 2006; the SiSEC 2018 form), for one source, one channel and one window over the whole file, restated in NumPy float64 from
the definition in include/vfx.h: what vfx_bsseval (voicefixer_main_amd/csrc/bsseval.hip) is held against, one function per stage.
A restatement: museval, mir_eval and speechmetrics are not pinned against.  `target` is r, `est` is e.

  a[k] = sum_t r[t] r[t + k],  d[k] = sum_t e[t] r[t - k],  k < flen          (terms outside [0, n) are zero)
  (toeplitz(a) + EPS I) c = d,  P = c * r over t < n + flen - 1
  sdr = 10 log10(sum r^2 / sum (e - r)^2), isr = 10 log10(sum r^2 / sum (P - r)^2), sar = 10 log10(sum P^2 / sum (e - P)^2)

The second solver (Levinson, scipy.linalg.solve_toeplitz) and the correlations by FFT are here only to measure how well defined the
scores are.  The input makers draw from numpy.random.default_rng(seed) and round to float32."""
import numpy as np
from scipy.linalg import solve_toeplitz, toeplitz
from scipy.signal import butter, lfilter

EPS = 2.0 ** -52
FLEN = 512
KEYS = ("sdr", "isr", "sar")


# ---------------------------------------------------------------------- 1, 2  the correlations
def _f64(x):
    return np.asarray(x, np.float64)


def correlations(est, target, flen=FLEN):
    """(a, d) by direct sums."""
    e, r = _f64(est), _f64(target)
    n = len(r)
    a, d = np.zeros(flen), np.zeros(flen)
    for k in range(min(flen, n)):
        a[k] = np.dot(r[:n - k], r[k:])
        d[k] = np.dot(e[k:], r[:n - k])
    return a, d


def correlations_fft(est, target, flen=FLEN):
    e, r = _f64(est), _f64(target)
    nfft = 1 << int(np.ceil(np.log2(len(r) + flen)))
    R, E = np.fft.rfft(r, nfft), np.fft.rfft(e, nfft)
    return np.fft.irfft(R * np.conj(R), nfft)[:flen], np.fft.irfft(E * np.conj(R), nfft)[:flen]


def correlation_terms(est, target, flen=FLEN):
    """Per lag of (a, d): the sum in numpy.longdouble (the products of float32 values are exact in float64), the sum of the terms'
    magnitudes and the count of terms -> three (2, flen) arrays."""
    e, r = _f64(est), _f64(target)
    n = len(r)
    exact, mag, cnt = np.zeros((2, flen), np.longdouble), np.zeros((2, flen)), np.zeros((2, flen), np.int64)
    for k in range(min(flen, n)):
        for s, x in enumerate((r, e)):
            t = x[k:] * r[:n - k]
            exact[s, k], mag[s, k], cnt[s, k] = np.sum(t.astype(np.longdouble)), np.sum(np.abs(t)), n - k
    return exact, mag, cnt


# ---------------------------------------------------------------------- 3  the filter
def gram(a):
    return toeplitz(a) + EPS * np.eye(len(a))


def solve_lu(a, d):
    return np.linalg.solve(gram(a), d)


def solve_levinson(a, d):
    col = np.array(a, np.float64)
    col[0] += EPS
    return solve_toeplitz(col, d)


def residual_ratio(a, d, c):
    """|| G c - d ||_inf / (flen 2^-53 (|| G ||_inf || c ||_inf + || d ||_inf)), G c in numpy.longdouble."""
    G = gram(a)
    res = np.abs(G.astype(np.longdouble) @ np.asarray(c, np.longdouble) - np.asarray(d, np.longdouble)).max()
    scale = len(a) * 2.0 ** -53 * (np.abs(G).sum(axis=1).max() * np.abs(c).max() + np.abs(d).max())
    return float(res / scale)


# ---------------------------------------------------------------------- 4, 5, 6  projection, energies, scores
def project(c, target):
    return np.convolve(_f64(c), _f64(target))           # n + flen - 1 samples


def energies(est, target, P):
    m = len(P)
    r, e = np.zeros(m), np.zeros(m)
    r[:len(target)], e[:len(est)] = target, est
    return np.array([np.sum(r * r), np.sum((e - r) ** 2), np.sum((P - r) ** 2), np.sum(P * P), np.sum((e - P) ** 2)])


def _db(num, den):
    if den == 0.0:
        return np.inf
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(num / den))


def scores(en):
    Err, Eer, Epr, Epp, Eep = en
    return np.array([_db(Err, Eer), _db(Err, Epr), _db(Epp, Eep)])


def bsseval(est, target, flen=FLEN, solver=solve_lu, corr=correlations):
    """-> (sdr, isr, sar); three NaN for a silent est or target."""
    est, target = _f64(est), _f64(target)
    if est.shape != target.shape or est.ndim != 1:
        raise ValueError("bsseval: est %s and target %s must be equal 1-D signals" % (est.shape, target.shape))
    if not np.any(target) or not np.any(est):
        return np.full(3, np.nan)
    a, d = corr(est, target, flen)
    return scores(energies(est, target, project(solver(a, d), target)))


def solver_spread(est, target, flen=FLEN):
    """The largest difference of a score between (LU, direct sums) and (Levinson, FFT correlations), dB."""
    return float(np.max(np.abs(bsseval(est, target, flen) - bsseval(est, target, flen, solve_levinson, correlations_fft))))


# ---------------------------------------------------------------------- the input makers: -> (est, target) float32
def _f32(*xs):
    return tuple(np.asarray(x, np.float64).astype(np.float32) for x in xs)


def make_a(n, seed, scale=1.0):
    """white target; est = the target through a 40-tap decaying random FIR + 0.1 white.  scale: the level of both, a power of two
    (the float32 samples of another level are the same numbers with another exponent)."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(n)
    h = rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0)
    e, t = _f32(np.convolve(t, h)[:n] + 0.1 * rng.standard_normal(n), t)
    return e * np.float32(scale), t * np.float32(scale)


def make_b(n, seed):
    """est = 0.5 target + 0.3 white"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(n)
    return _f32(0.5 * t + 0.3 * rng.standard_normal(n), t)


def make_c(n, seed):
    """coloured target (butter(2, 0.5) of white + 0.05 white); est = 0.8 x the target delayed by 3 + 0.05 white"""
    rng = np.random.default_rng(seed)
    b, a = butter(2, 0.5)
    t = lfilter(b, a, rng.standard_normal(n)) + 0.05 * rng.standard_normal(n)
    e = 0.05 * rng.standard_normal(n)
    e[3:] += 0.8 * t[:n - 3]
    return _f32(e, t)


def make_s(n=44100, seed=0):
    """the speech-like pair: butter(8, 8000 / 22050) low-passed white; est = target + 0.01 white"""
    rng = np.random.default_rng(seed)
    b, a = butter(8, 8000.0 / 22050.0)
    t = lfilter(b, a, rng.standard_normal(n))
    return _f32(t + 0.01 * rng.standard_normal(n), t)


MAKERS = {"A": make_a, "B": make_b, "C": make_c}

# ---------------------------------------------------------------------- the cases of the GPU test
FLENS = (16, 48, 512)
# seed 1 unless the pair it gives breaks a condition tests/test_bsseval_host.py asserts (cond(toeplitz(a)) <= 1e4 here)
SEEDS = {("C", 513, 512): 6}


def lengths(slab):
    """n < flen, n not a multiple of 4 or 16, both sides of a slab boundary of the kernels, more than two slabs."""
    return (5, 15, 17, 511, 513, 700, slab - 1, slab + 1, 2 * slab + 3, 20000)


def cases(slab):
    """[(maker, seed, n, flen)]"""
    return [(m, SEEDS.get((m, n, f), 1), n, f) for f in FLENS for m in sorted(MAKERS) for n in lengths(slab)]


def pair(maker, seed, n):
    return MAKERS[maker](n, seed)


# The EPS of the definition is absolute, everything else scales with the level: at unit level it is under half an ulp of a[0] = sum r^2
# and toeplitz(a) + EPS I is toeplitz(a) bit for bit.  It counts for a quiet pair.  Input A at 2^-24 of unit level (-144 dB): EPS is 1e-4
# of a[0] at n = 700, and leaving it off moves isr and sar by 1e-3 dB.  One slab and more than two; one and two accumulators.
QUIET = 2.0 ** -24
QUIET_CASES = ((1, 700, 48), (1, 700, 512), (1, 20000, 512))         # (seed, n, flen) of make_a(n, seed, QUIET)


def quiet_pair(seed, n):
    return make_a(n, seed, QUIET)
