"""STOI (Taal, Hendriks, Heusdens, Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy Speech",
IEEE TASLP 2011) restated in NumPy float64 from the paper, the authors' MATLAB and pystoi's stoi(extended=False): what vfx_stoi
(voicefixer_main_amd/csrc/stoi.hip) is held against, one function per stage.  `target` is the clean signal (pystoi's x), `est` the
processed one (y); the score is not symmetric.

Frame-count convention: frames start at range(0, n - 256, 128) in the silent-frame removal and in the STFT (the authors'
1:hop:(length - N)): the last aligned frame is not taken."""
import math

import numpy as np
from scipy.signal import resample_poly

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
N_BANDS = 15
MIN_FREQ = 150.0
SEG = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
SHORT_SCORE = 1e-5      # fewer than SEG frames after the silent-frame removal (pystoi's warning value)


# ---------------------------------------------------------------------- 1  resampling (Octave's resample filter)
def ratio(fs):
    g = math.gcd(FS, int(fs))
    return FS // g, int(fs) // g


def filter_half_length(up, down):
    fc = 1.0 / (2 * max(up, down))
    return int(math.ceil((60.0 - 8.0) / (28.714 * (fc / 10.0))))


def resample_filter(up, down):
    """h of Octave's resample for up/down (reduced): Kaiser-windowed sinc, 60 dB rejection, roll-off width fc / 10."""
    fc = 1.0 / (2 * max(up, down))
    L = filter_half_length(up, down)
    t = np.arange(-L, L + 1)
    return np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * (2 * up * fc * np.sinc(2 * fc * t))


def resample_taps(up, down):
    """What resample_poly(x, up, down, window=h / sum(h)) filters with: up * h / sum(h)."""
    h = resample_filter(up, down)
    return up * (h / np.sum(h))


def resample(x, fs):
    x = np.asarray(x, np.float64)
    if int(fs) == FS:
        return x
    up, down = ratio(fs)
    h = resample_filter(up, down)
    return resample_poly(x, up, down, window=h / np.sum(h))


def resample_terms(x, up, down):
    """Per output of `resample`: (K, sum_k |x_k h_k|) over that output's own terms."""
    x = np.asarray(x, np.float64)
    h = resample_filter(up, down)
    w = h / np.sum(h)
    K = np.rint(resample_poly(np.ones(len(x)), up, down, window=np.ones(len(h)) / up)).astype(np.int64)
    return K, resample_poly(np.abs(x), up, down, window=np.abs(w))


# ---------------------------------------------------------------------- 2  silent-frame removal
def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_starts(n):
    return range(0, n - N_FRAME, HOP)


def frames_of(x):
    """(frames, 256): the windowed frames of x."""
    w = window()
    return np.array([w * x[i:i + N_FRAME] for i in frame_starts(len(x))]).reshape(-1, N_FRAME)


def frame_energies(target):
    return 20.0 * np.log10(np.linalg.norm(frames_of(target), axis=1) + EPS)


def keep_mask(target):
    e = frame_energies(target)
    if len(e) == 0:
        return np.zeros(0, bool)
    return (np.max(e) - DYN_RANGE - e) < 0


def overlap_add(frames):
    out = np.zeros((len(frames) - 1) * HOP + N_FRAME if len(frames) else 0)
    for i, f in enumerate(frames):
        out[i * HOP:i * HOP + N_FRAME] += f
    return out


def remove_silent_frames(est, target):
    """-> (est, target) with the frames whose TARGET energy is 40 dB or more under the loudest one taken out."""
    mask = keep_mask(target)
    return overlap_add(frames_of(est)[mask]), overlap_add(frames_of(target)[mask])


# ---------------------------------------------------------------------- 3, 4  STFT and third-octave bands
def stft(x):
    """(frames, 257) complex."""
    return np.fft.rfft(frames_of(x), n=NFFT, axis=1).reshape(-1, NFFT // 2 + 1)


def band_edges():
    """[(lo, hi)] rFFT bins, half-open: the bins nearest to 150 * 2^((2 j -+ 1) / 6) Hz."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    j = np.arange(N_BANDS)
    lo = MIN_FREQ * 2.0 ** ((2 * j - 1) / 6.0)
    hi = MIN_FREQ * 2.0 ** ((2 * j + 1) / 6.0)
    return [(int(np.argmin(np.square(f - a))), int(np.argmin(np.square(f - b)))) for a, b in zip(lo, hi)]


def band_powers(x):
    """(15, frames): the summed |X|^2 of each band per STFT frame of x."""
    p = np.square(np.abs(stft(x)))
    return np.array([p[:, a:b].sum(axis=1) for a, b in band_edges()]).reshape(N_BANDS, -1)


def tob(x):
    return np.sqrt(band_powers(x))


# ---------------------------------------------------------------------- 5  the score
def score(est_tob, target_tob):
    """(15, M) band matrices -> d; SHORT_SCORE when M < 30."""
    M = target_tob.shape[1]
    if M < SEG:
        return SHORT_SCORE
    x = np.array([target_tob[:, m - SEG:m] for m in range(SEG, M + 1)])     # (segments, 15, 30)
    y = np.array([est_tob[:, m - SEG:m] for m in range(SEG, M + 1)])
    alpha = np.linalg.norm(x, axis=2, keepdims=True) / (np.linalg.norm(y, axis=2, keepdims=True) + EPS)
    yp = np.minimum(alpha * y, x * (1.0 + 10.0 ** (-BETA / 20.0)))
    yp = yp - np.mean(yp, axis=2, keepdims=True)
    x = x - np.mean(x, axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    x = x / (np.linalg.norm(x, axis=2, keepdims=True) + EPS)
    return float(np.sum(yp * x) / (x.shape[0] * N_BANDS))


def stoi(est, target, fs=FS):
    est, target = np.asarray(est, np.float64), np.asarray(target, np.float64)
    if est.shape != target.shape or est.ndim != 1:
        raise ValueError("stoi: est %s and target %s must be equal 1-D signals" % (est.shape, target.shape))
    e, t = remove_silent_frames(resample(est, fs), resample(target, fs))
    return score(tob(e), tob(t))
