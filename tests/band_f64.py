"""Shared by tests/test_band_host.py and tests/test_gpu_band.py: the float64 restatement of the bandwidth detector (csrc/band.hip;
load_wav_energy of tools/utils.py:33-44), the clips the two files use, the bound of the GPU tests and the margin a clip's discrete
decision must have.  A plain helper module, no tests.

The spectrogram is oracle.dsp.stft(x, 2048, hop) (periodic Hann, centred frames, reflect padding: librosa.stft's reading, as
tests/audio_metrics_f64.py); the five steps are restated from the reference source:
  1  S = stft(x): T = 1 + L // hop frames, 1025 bins, |S| = sqrt(re^2 + im^2), no eps clamp
  2  e[k] = sum_t log10(|S[k, t]| + 1)
  3  P[k] = sum_{j<k} e[j] (the loop of utils.py:38-39 runs from the top down: the EXCLUSIVE prefix); total = P[1024]
  4  i = the first index that does not have P[i] < total * threshold
  5  Hz = int((sample_rate // 2) * (i / 1025))
`profile` and `decide` have switches that plant the defects a padded-batch kernel can have; the host test shows that each moves e by
more than the GPU tests allow, or moves the bin."""
import math

import numpy as np

from oracle import dsp

NFFT = 2048
NBINS = 1025
HOP = 512                     # librosa.stft's default
THRESHOLD = 0.95
U32 = 2.0 ** -24
U64 = 2.0 ** -53
AMP = 0.05                    # the partials of make_clip, together
L65 = 28241
LENGTHS = (1025, 1322, 1323, 2048, 4533, L65)      # 3 .. 56 frames at hop 512: fewer and more than a wave walks, L mod hop zero and not
# make_clip seeds, of 0-11 the one with the widest margin at hop 512 and 441: margin / bound = 14, 69, 65, 66, 71, 77
SEEDS = {1025: 0, 1322: 4, 1323: 10, 2048: 0, 4533: 7, L65: 0}
MARGIN_FACTOR = 10.0


def frames(n, hop=HOP):
    return n // hop + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# clips
# ---------------------------------------------------------------------------------------------------------------------------------
def make_clip(n, seed):
    """float32 (n,): seven cosine partials at 300-9000 Hz, AMP in total, under a 0.5 -> 1 ramp (the last samples differ from the first: a
    reflection at the wrong place shows), over a noise floor of 1e-7 (the upper bins lie far below the 1e-4 an eps clamp would put
    there).  The frequencies are multiples of 44100 / (2 (n - 1)): every partial has an extremum at both ends of the clip, so the
    reflect padding continues it without a kink.  A kink's 1 / f^2 skirt -- log10(|S| + 1) is linear in small magnitudes -- would hold
    more than the last 5 % of a short clip's energy, and the 95 % level would fall among bins of almost no energy, where no
    decision has a margin; without it the level falls inside the top partial's lobe."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    step = 44100.0 / (2 * (n - 1))
    m = rng.integers(int(np.ceil(300.0 / step)), int(9000.0 / step) + 1, size=7)
    x = (AMP / 7.0) * np.linspace(0.5, 1.0, n) * sum(np.cos(2.0 * np.pi * (mi * step) * t) for mi in m)
    return (x + 1e-7 * rng.standard_normal(n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 forms
# ---------------------------------------------------------------------------------------------------------------------------------
def magnitude(clip, hop=HOP, eps=0.0, row=None, row_frames=False):
    """|STFT| of a clip (n,) -> (frames, 1025) float64.  DEFECTS: eps > 0 (the clamp on the power left in), row (the clip sits in a
    zero-padded row of that many samples and is framed and reflected as the row; its own frame count is kept), row_frames (... and
    the row's frame count is used)."""
    x = np.asarray(clip, np.float64)
    n = x.shape[0]
    if row is not None:
        x = np.concatenate([x, np.zeros(row - n)])
    re, im = dsp.stft(x[None], NFFT, hop)
    mag = np.sqrt(np.maximum(re[0] ** 2 + im[0] ** 2, eps))
    return mag if row_frames else mag[:frames(n, hop)]


def profile(clip, hop=HOP, **defects):
    """steps 1-2: e (1025,) float64"""
    return np.log10(magnitude(clip, hop, **defects) + 1.0).sum(axis=0)


def decide(e, threshold=THRESHOLD, inclusive=False, count_top=False):
    """steps 3-4 -> (i, P (1025,), level = total * threshold).  DEFECTS: inclusive (P[k] = sum_{j<=k} e[j]), count_top (bin 1024 counted:
    total = the sum of all 1025)."""
    e = np.asarray(e, np.float64)
    P = np.concatenate([[0.0], np.cumsum(e)[:-1]])
    total = P[-1] + (e[-1] if count_top else 0.0)
    if inclusive:
        P = P + e
    level = total * threshold
    for i in range(NBINS):
        if not P[i] < level:
            return i, P, level
    return NBINS - 1, P, level


def cut_bin(clip, hop=HOP, threshold=THRESHOLD):
    return decide(profile(clip, hop), threshold)[0]


def hz(i, sample_rate=44100):
    """step 5"""
    return int((sample_rate // 2) * (i / NBINS))


def cutoff(clip, sample_rate=44100, hop=HOP, threshold=THRESHOLD):
    return hz(cut_bin(clip, hop, threshold), sample_rate)


# ---------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests compare with, and how closely
# ---------------------------------------------------------------------------------------------------------------------------------
def energy_bound(clip, hop=HOP):
    """|e_gpu[k] - e[k]| <= this, for every k.  The device's transform is float32: a radix-2-equivalent transform of 2048 points errs by
    at most 11 * 2^-24 * A_t per bin, A_t = sum_n |x_n w_n| of frame t (the bound tests/test_gpu_val_losses.py uses); |.| is
    1-Lipschitz and d/dm log10(m + 1) <= 1 / ln 10, so a frame's term moves by at most 11 * 2^-24 * A_t / ln 10.  On top: the float64
    logarithm (2 ulp of a term <= log10(A_t + 1)) and the float64 sum of T terms in any order (T u times their sum)."""
    x = np.asarray(clip, np.float64)
    A = np.abs(dsp.frame_signal(x[None], NFFT, hop)[0] * dsp.hann_periodic(NFFT)).sum(axis=1)      # (T,)
    terms = np.log10(A + 1.0)                                                                       # >= any bin's term of the frame
    return float((11.0 * U32 * A / math.log(10.0)).sum() + 2.0 * np.spacing(terms).sum() + A.size * U64 * terms.sum())


def decision_bounds(clip, hop=HOP, threshold=THRESHOLD):
    """(i, margin, bound): the distance of level = threshold * total from P[i] and from P[i - 1], and the bound of P[i] plus that of the
    level -- i (1024 at the most) terms and threshold * 1024 terms of energy_bound each, and the float64 prefix sum itself."""
    e = profile(clip, hop)
    i, P, level = decide(e, threshold)
    be = energy_bound(clip, hop)
    chain = NBINS * U64 * P[-1]
    margin = P[i] - level if i == 0 else min(P[i] - level, level - P[i - 1])
    return i, float(margin), float(i * be + chain + threshold * ((NBINS - 1) * be + chain))


def decision_margin(clip, hop=HOP, threshold=THRESHOLD):
    return decision_bounds(clip, hop, threshold)[1]


def checked(clip, hops=(HOP,), threshold=THRESHOLD):
    """The clip, once its decision is safe to compare exactly at every hop: margin >= MARGIN_FACTOR x the bound.  A condition on the
    test's input, not a tolerance: a clip that fails it is an error in the test's inputs."""
    for hop in hops:
        i, margin, bound = decision_bounds(clip, hop, threshold)
        assert margin >= MARGIN_FACTOR * bound, ("test-input error: decision too close to a bin's edge", len(clip), hop, i, margin, bound)
    return clip


def clip_for(n, hops=(HOP, 441)):
    """The test clip of n samples (n in LENGTHS), its margin asserted at every hop in `hops`."""
    return checked(make_clip(n, SEEDS[n]), hops)
