"""Shared by tests/test_val_losses_host.py and tests/test_gpu_val_losses.py: the float64 forms of the validation losses (csrc/losses.hip:
L1, L1_Sp and L1_Log_Sp of tools/pytorch/losses.py:178-204, 273-279, and val_l of models/gsr_voicefixer.py:264-277), the clips the two
files use, and the summation bound of the GPU tests.  A plain helper module, no tests.

The spectrogram is oracle.dsp's (which the goldens pin to the reference's own STFT); the formulas are restated from the reference
source.  Each function takes ONE clip pair -- the reference validates with batch_size = 1 -- and has switches that plant the defects a
padded-batch implementation can have; the host test shows that each moves the value by more than the GPU tests allow."""
import numpy as np

from oracle import dsp

HOP = 441
NFFT = 2048
NBINS = 1025
NMEL = 128
EPS = 1e-8
U64 = 2.0 ** -53
AMP = 0.004                   # the partials of make_pair


def frames(n):
    return n // HOP + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# clips
# ---------------------------------------------------------------------------------------------------------------------------------
def make_pair(n, seed):
    """(est, target) float32 (n,): a few partials below 5 kHz at amplitude AMP over a noise floor of 1e-6, so that in every clip --
    the shortest included, whose frames are mostly reflection -- upper bins of the spectra lie below the clamp (power < 1e-8: dropping
    eps shows in every clip) while the lower ones are far above it; est is the target scaled, detuned and with a floor of its own.
    The last samples differ from the first: a reflection at the wrong place shows."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    f = rng.uniform(200.0, 5000.0, size=4)
    ramp = np.linspace(0.3, 1.0, n)
    tgt = AMP * ramp * sum(np.sin(2 * np.pi * fi * t + p) for fi, p in zip(f, rng.uniform(0, 6.28, size=4))) / 4
    est = 0.8 * tgt + 0.2 * AMP * ramp[::-1] * np.sin(2 * np.pi * 1.07 * f[0] * t)
    tgt = tgt + 1e-6 * rng.standard_normal(n)
    est = est + 1e-6 * rng.standard_normal(n)
    return est.astype(np.float32), tgt.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 forms
# ---------------------------------------------------------------------------------------------------------------------------------
def magnitude(clip, eps=EPS, row=None):
    """|STFT| of a clip (n,) -> (frames(n), 1025) float64: FDomainHelper.wav_to_spectrogram(eps).  row: DEFECT -- the clip sits in a
    zero-padded row of that many samples and is framed and reflected as the row (its own frame count is kept)."""
    x = np.asarray(clip, np.float64)
    n = x.shape[0]
    if row is not None:
        x = np.concatenate([x, np.zeros(row - n)])
    mag = dsp.spectrogram_phase(x[None, None], eps=eps)[0][0, 0]
    return mag[:frames(n)]


def l1_wav(est, tgt):
    return float(np.abs(np.asarray(est, np.float64) - np.asarray(tgt, np.float64)).mean())


def l1_sp(est, tgt, eps=EPS, row=None, denominator_frames=None):
    """L1_Sp (losses.py:192-204).  DEFECTS: eps = 0 (the clamp dropped), row (reflection at the row's end), denominator_frames (the
    mean over that many frames, the batch's, in place of the clip's own)."""
    d = np.abs(magnitude(est, eps, row) - magnitude(tgt, eps, row))
    return float(d.sum() / ((denominator_frames or d.shape[0]) * NBINS))


def l1_log_sp(est, tgt, eps=EPS, row=None, denominator_frames=None, log_of_mean=False):
    """L1_Log_Sp (losses.py:178-190).  DEFECT log_of_mean: |log10 mean_f se - log10 mean_f st| per frame in place of the mean over the
    bins of |log10 se - log10 st|."""
    se, st = magnitude(est, eps, row), magnitude(tgt, eps, row)
    with np.errstate(divide="ignore", invalid="ignore"):
        if log_of_mean:
            return float(np.abs(np.log10(se.mean(axis=1)) - np.log10(st.mean(axis=1))).mean())
        d = np.abs(np.log10(se) - np.log10(st))
    return float(d.sum() / ((denominator_frames or d.shape[0]) * NBINS))


def target_logmel(tgt, row=None):
    """to_log(mel(target)) (gsr_voicefixer.py:266, 269) -> (frames(n), 128) float64"""
    return dsp.to_log(dsp.mel_project(magnitude(tgt, EPS, row), dsp.mel_filterbank().astype(np.float64)))


def val_l(logmel_est, tgt, row=None, denominator_frames=None):
    """val_l (gsr_voicefixer.py:264-270): L1 of the model's log-mel estimate (frames(n), 128) and to_log(mel(target))"""
    d = np.abs(np.asarray(logmel_est, np.float64) - target_logmel(tgt, row))
    return float(d.sum() / ((denominator_frames or d.shape[0]) * NMEL))


def mixed(wav, sp, alpha_t=0.85, window_size=2048):
    """L1_Wav_L1_Sp / L1_Wav_L1_Log_Sp (losses.py:227-237, 260-270)"""
    return alpha_t * wav + (1 - alpha_t) * (sp / np.sqrt(window_size))


# ---------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests compare with, and how closely
# ---------------------------------------------------------------------------------------------------------------------------------
def sum_bound(terms):
    """A float64 sum of the n non-negative `terms` in ANY order differs from the exact sum by at most (n - 1) u sum|terms| to first
    order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), u = 2^-53; the tests allow n u sum|terms|, which also covers
    the division by the count and the host's own sum."""
    terms = np.asarray(terms, np.float64)
    return terms.size * U64 * float(np.abs(terms).sum())


def mean_abs_f32_diff(a32, b32):
    """(mean |float32(a - b)|, its bound): the float32 subtraction the kernel does, then float64 -- of two float32 arrays"""
    a32, b32 = np.asarray(a32), np.asarray(b32)
    assert a32.dtype == np.float32 and b32.dtype == np.float32
    terms = np.abs(a32 - b32).astype(np.float64)
    return float(terms.sum() / terms.size), sum_bound(terms) / terms.size


def mean_abs_log_diff(a32, b32):
    """(mean |log10 a - log10 b| in float64 of two float32 arrays, its bound): two ulp64 of each logarithm on top of the summation"""
    a, b = np.asarray(a32).astype(np.float64), np.asarray(b32).astype(np.float64)
    la, lb = np.log10(a), np.log10(b)
    terms = np.abs(la - lb)
    ulp = 2.0 * (np.spacing(np.abs(la)) + np.spacing(np.abs(lb)))
    return float(terms.sum() / terms.size), (sum_bound(terms) + float(ulp.sum())) / terms.size
