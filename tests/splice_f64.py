"""Shared by tests/test_splice_host.py and tests/test_gpu_splice.py: the float64 restatement of the splice (csrc/stft.hip k_stft_splice;
voicefixer_main_amd/splice.py) over oracle.dsp.spectrogram_phase and oracle.dsp.istft, its weight, band and gain rules written a second
time, the two-spectrum blend it equals by linearity, the tolerance the GPU test holds the kernel to, and planted defects that tolerance
has to see."""
import math

import numpy as np

from oracle import dsp

NBINS = 1025
HOP = 441

DEFECTS = ("ramp_off_by_one", "weights_swapped", "gain_not_in_sum", "padded_reflection")


def weights(c, w):
    """a[k] = 1 for k <= c - w - 1, 0 for k >= c, (c - k) / (w + 1) between: the line through (c, 0) with slope -1 / (w + 1), clipped."""
    k = np.arange(NBINS, dtype=np.float64)
    return np.clip((float(c) - k) / float(w + 1), 0.0, 1.0)


def _spectrum(sig):
    """(n,) float64 -> (re, im) each (T, 1025), formed as lowpass_spectrum forms them: mag cos, mag sin (eps 1e-8)"""
    mag, cos, sin = dsp.spectrogram_phase(sig[None, None], dtype=np.float64)
    return (mag * cos)[0, 0], (mag * sin)[0, 0]


def splice(x, y, c, w, g=1.0, defect=None, row_len=None):
    """Steps 1-6 of the definition in float64: x, y (n,) -> out (n,).  g is taken as the float32 the kernel receives.  `defect`: one of
    DEFECTS; "padded_reflection" needs row_len > n, the width of the zero-padded row the wrong reflection would be taken from."""
    assert defect is None or defect in DEFECTS
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.shape[0]
    g = float(np.float32(g))
    gy = g * y                                            # 1
    d = x - gy                                            # 2
    a = weights(c + 1 if defect == "ramp_off_by_one" else c, w)      # 3
    if defect == "weights_swapped":
        a = 1.0 - a
    if defect == "padded_reflection":
        assert row_len is not None and row_len > n
        re, im = _spectrum(np.concatenate([d, np.zeros(row_len - n)]))
        re, im = re[:n // HOP + 1], im[:n // HOP + 1]
    else:
        re, im = _spectrum(d)                             # 4
    r = dsp.istft((re * a)[None], (im * a)[None], n, dtype=np.float64)[0]      # 5
    return (y if defect == "gain_not_in_sum" else gy) + r                      # 6


def blend(x, y, c, w, g=1.0):
    """ISTFT(a STFT(x) + (1 - a) STFT(g y)): what the splice is by linearity, with two forward transforms"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    a = weights(c, w)
    xr, xi = _spectrum(x)
    yr, yi = _spectrum(float(np.float32(g)) * y)
    return dsp.istft((a * xr + (1.0 - a) * yr)[None], (a * xi + (1.0 - a) * yi)[None], x.shape[0], dtype=np.float64)[0]


def tolerance(x, y, g, ref):
    """What the kernel may differ from `splice` by, per sample: 2e-5 * max(1, max |d|) for the masked float32 round trip of d (the bound
    tests/test_gpu_stft_lowpass.py holds that round trip to), plus 2^-22 * max(|g y|, |ref|) for the three float32 roundings outside it
    (the product g y, the subtraction, the final sum)."""
    gy = float(np.float32(g)) * np.asarray(y, np.float64)
    d = np.asarray(x, np.float64) - gy
    return 2e-5 * max(1.0, float(np.abs(d).max())) + 2.0 ** -22 * np.maximum(np.abs(gy), np.abs(ref))


def match_band(c, w, match):
    """The `match` bins just under the ramp, never the first five"""
    hi = c - w
    lo = hi - match
    lo = 5 if lo < 5 else lo
    return lo, (lo if hi < lo else hi)


def match_gain(p_in, p_out, n_terms, max_gain_db):
    """sqrt(p_in / p_out) within +-max_gain_db, as a float32; 1 for an empty or silent band"""
    if n_terms == 0 or p_in <= 4e-8 * n_terms or p_out <= 4e-8 * n_terms:
        return 1.0
    db = 10.0 * math.log10(p_in / p_out)
    db = max(-max_gain_db, min(max_gain_db, db))
    return float(np.float32(10.0 ** (db / 20.0)))


def band_power(x, lo, hi):
    """sum over the frames and the bins lo <= k < hi of max(re^2 + im^2, 1e-8), float64"""
    mag, _, _ = dsp.spectrogram_phase(np.asarray(x, np.float64)[None, None], dtype=np.float64)
    return float((mag[0, 0, :, lo:hi] ** 2).sum())
