"""float64 numpy restatement of AudioMetrics.evaluation's nine scores (evaluation_proc/metrics.py:25-106) for the scoring tests.

Spectrogram: np.abs(librosa.stft(wav, n_fft=2048, hop_length=441)) = oracle.dsp.stft (periodic Hann, centre reflect padding) with
no eps clamp; mel: MelScale(128, 44100, 1025) = oracle.dsp.mel_filterbank; LSD / SiSpec: oracle.metrics; SSIM: skimage 0.18's
structural_similarity(win_size=7) for float images (uniform_filter, sample covariance, K1 0.01, K2 0.03, data_range 2, the
(win_size - 1) // 2 border cropped); SI-SDR: speechmetrics' relative/sisdr.py as recalled (the package is not available to pin it).
"""
import numpy as np
from scipy.ndimage import uniform_filter

from oracle import dsp
from oracle import metrics as om

KEYS = ("sisdr", "lsd", "non_log_sispec", "sispec", "ssim",
        "final_mel_lsd", "final_non_log_mel_sispec", "final_mel_sispec", "final_mel_ssim")


def spectrogram(wav):
    """(L,) -> |STFT| (1 + L // 441, 1025) float64."""
    re, im = dsp.stft(np.asarray(wav, np.float64)[None])
    return np.sqrt(re[0] ** 2 + im[0] ** 2)


def mel(sp):
    return sp @ dsp.mel_filterbank(dtype=np.float64)


def to_log(x):
    return np.log10(np.clip(x, 1e-8, None))


def lsd(est, target):
    """(T, F) images -> metrics.py:83-87 for one clip."""
    return float(om.lsd(est[None, None], target[None, None])[0, 0])


def sispec(est, target):
    return float(om.sispec_per_clip(est[None, None], target[None, None])[0])


def ssim(x, y, win=7, data_range=2.0, k1=0.01, k2=0.03):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if min(x.shape) < win:
        raise ValueError("win_size exceeds image extent")
    n = win * win
    cov = n / (n - 1.0)
    ux, uy = uniform_filter(x, win), uniform_filter(y, win)
    uxx, uyy, uxy = uniform_filter(x * x, win), uniform_filter(y * y, win), uniform_filter(x * y, win)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    p = (win - 1) // 2
    return float(s[p:-p, p:-p].mean())


def ssim_brute(x, y, win=7, data_range=2.0, k1=0.01, k2=0.03):
    """The same by an explicit loop over the windows that lie inside the image."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    vals = []
    for i in range(x.shape[0] - win + 1):
        for j in range(x.shape[1] - win + 1):
            a, b = x[i:i + win, j:j + win].ravel(), y[i:i + win, j:j + win].ravel()
            ma, mb = a.mean(), b.mean()
            va, vb = a.var(ddof=1), b.var(ddof=1)
            cab = ((a - ma) * (b - mb)).sum() / (a.size - 1)
            vals.append(((2 * ma * mb + c1) * (2 * cab + c2)) / ((ma ** 2 + mb ** 2 + c1) * (va + vb + c2)))
    return float(np.mean(vals))


def sisdr(est, ref):
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    eps = np.finfo(np.float64).eps
    a = (eps + np.dot(ref, est)) / (np.dot(ref, ref) + eps)
    e_true = a * ref
    sss = np.sum(e_true ** 2)
    snn = np.sum((est - e_true) ** 2)
    return float(10 * np.log10((eps + sss) / (eps + snn)))


def audio_metrics(est, target):
    """Waveforms (L,) -> the nine scores in KEYS order."""
    es, ts = spectrogram(est), spectrogram(target)
    em, tm = mel(es), mel(ts)
    out = [sisdr(est, target)]
    for e, t in ((es, ts), (em, tm)):
        out += [lsd(e, t), sispec(e, t), sispec(to_log(e), to_log(t)), ssim(e, t)]
    return np.array(out)
