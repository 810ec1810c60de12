"""float64 numpy restatement of the 16 kHz branch of AudioMetrics.evaluation (evaluation_proc/metrics.py:37-51) for the scoring tests.

Spectrogram: np.abs(librosa.stft(wav, n_fft=743, hop_length=160)): periodic Hann of 743 points, centre reflect padding.  An odd n_fft
pads n_fft // 2 = 371 samples on each side -- 742 in all, not n_fft -- so a clip of L samples has 1 + (L - 1) // 160 frames: one
fewer than L // 160 + 1 when L is a multiple of 160.  (oracle.dsp.frame_signal assumes an even n_fft; the framing is restated here.)
mel: MelScale(n_mels=80, sample_rate=16000, n_stft=372) = oracle.dsp.mel_filterbank(372, 80, 16000).  The scores are those of
tests/audio_metrics_f64.py on these two images.
"""
import numpy as np

from oracle import dsp

from audio_metrics_f64 import KEYS, lsd, sisdr, sispec, ssim, to_log  # noqa: F401

RATE, N_FFT, HOP, N_BINS, N_MELS = 16000, 743, 160, 372, 80
PAD = N_FFT // 2
MIN_SAMPLES = 6 * HOP + 1


def num_frames(length):
    return 1 + (length - 1) // HOP


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def frames(wav):
    """(L,) -> (T, 743) float64 frames of the reflect-padded clip, not windowed."""
    x = np.asarray(wav, np.float64)
    xp = np.pad(x, (PAD, PAD), mode="reflect")
    idx = np.arange(num_frames(len(x)))[:, None] * HOP + np.arange(N_FFT)[None, :]
    return xp[idx]


def spectrogram(wav):
    """(L,) -> |STFT| (1 + (L - 1) // 160, 372) float64."""
    return np.abs(np.fft.rfft(frames(wav) * window(), axis=-1))


def spectrogram_dft_matrix(wav, frame_ids):
    """The same for the frames `frame_ids` by an explicit DFT matrix (the angle index reduced as an integer)."""
    fr = frames(wav)[frame_ids] * window()
    ang = 2.0 * np.pi * ((np.arange(N_FFT)[:, None] * np.arange(N_BINS)[None, :]) % N_FFT) / N_FFT
    return np.hypot(fr @ np.cos(ang), fr @ np.sin(ang))


def filterbank():
    return dsp.mel_filterbank(N_BINS, N_MELS, RATE, dtype=np.float64)


def mel(sp):
    return sp @ filterbank()


def audio_metrics(est, target):
    """Waveforms (L,) at 16 kHz -> the nine scores in KEYS order."""
    es, ts = spectrogram(est), spectrogram(target)
    em, tm = mel(es), mel(ts)
    out = [sisdr(est, target)]
    for e, t in ((es, ts), (em, tm)):
        out += [lsd(e, t), sispec(e, t), sispec(to_log(e), to_log(t)), ssim(e, t)]
    return np.array(out)
