"""Shared by tests/test_gpu_frontend_launches.py and tests/test_frontend_f64_host.py: the float64 forms of the STFT / ISTFT front end
(csrc/stft.hip) and of the glue launches between the models of a restore call (csrc/small_ops.hip), the seeded inputs of the glue
cases, and the cases' shapes.  A plain helper module, no tests.

Every reference takes the float32 values the kernel receives, widened to float64, and restates nothing oracle/dsp.py, oracle/pipeline.py
or oracle/vocoder.py already state: a padded batch is the oracle's operation on each clip's own samples, laid out the way the varlen
callers lay it out (T = the row stride, rows past a clip's frames 0 or -8)."""
import numpy as np
import torch

from oracle import dsp
from oracle import vocoder as voc

HOP = 441
NFFT = 2048
NBINS = 1025
NMEL = 128
U32 = 2.0 ** -24
BAND_LO, BAND_HI = 5, 25          # amp_to_original_f: mel bins 5 .. int(128 * 0.2) - 1

# 1025: the shortest clip the reflection allows (3 frames); 1322 / 1323: one sample below and at 3 * 441, where a fourth frame appears;
# 1764 = 4 * 441; 2048 = n_fft; 2500; 4533: 11 frames, the longest
EDGE_LENGTHS = [1025, 1322, 1323, 1764, 2048, 2500, 4533]
L65 = 28241                       # 64 * 441 + 17: 65 frames, L mod hop != 0


def frames(n):
    return n // HOP + 1


_FB64 = None


def mel_fb64():
    global _FB64
    if _FB64 is None:
        _FB64 = dsp.mel_filterbank().astype(np.float64)     # the float32 table the handle holds, widened
    return _FB64


# ---------------------------------------------------------------------------------------------------------------------------------
# STFT / ISTFT
# ---------------------------------------------------------------------------------------------------------------------------------
def stft_ref(x, eps=1e-8, want=("sp", "re", "im", "mel")):
    """x (B, n) float32, every row a whole clip -> dict of float64 arrays (B, frames(n), .): sp = sqrt(max(re^2 + im^2, eps)),
    re = sp * cos, im = sp * sin (what the tests compare the phases through), mel = sp @ fb."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    mag, cos, sin = dsp.spectrogram_phase(x[:, None].astype(np.float64), eps=eps)
    mag = mag[:, 0]
    out = {}
    if "sp" in want:
        out["sp"] = mag
    if "re" in want:
        out["re"] = mag * cos[:, 0]
    if "im" in want:
        out["im"] = mag * sin[:, 0]
    if "mel" in want:
        # (rows as one matrix: numpy's stacked matmul runs this product some hundred times slower)
        out["mel"] = dsp.mel_project(mag.reshape(-1, NBINS), mel_fb64()).reshape(mag.shape[:-1] + (NMEL,))
    return out


def stft_ref_chunked(x, want=("mel",), chunk=64):
    """stft_ref over a large batch of equal-length clips, `chunk` clips at a time (the (B, T, 2048) float64 frames never exist at once)."""
    parts = [stft_ref(x[i:i + chunk], want=want) for i in range(0, x.shape[0], chunk)]
    return {k: np.concatenate([p[k] for p in parts]) for k in want}


def pad_rows(rows, T, fill):
    """Per-clip arrays (T_b, F) -> (B, T, F): clip b's rows, then `fill` (the rows the kernel writes past a clip's frames)."""
    out = np.full((len(rows), T) + rows[0].shape[1:], fill, rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :min(T, r.shape[0])] = r[:T]
    return out


def stft_ref_varlen(clips, T, eps=1e-8, want=("sp", "re", "im", "mel")):
    """A padded batch: clips = list of float32 (n_b,) -> dict of (B, T, .) float64, rows past frames(n_b) zero."""
    per = [stft_ref(c[None], eps, want) for c in clips]
    return {k: pad_rows([p[k][0] for p in per], T, 0.0) for k in want}


def to_log(mel):
    """log10(max(mel, 1e-8)) (dsp.to_log)"""
    return dsp.to_log(mel)


def spectrum32(clip):
    """The float64 STFT of a float32 clip, rounded to float32: the input of the ISTFT cases -> re, im (frames, 1025) float32."""
    re, im = dsp.stft(clip[None].astype(np.float64))
    return re[0].astype(np.float32), im[0].astype(np.float32)


def istft_ref(re32, im32, length):
    """dsp.istft of float32 spectra (B, T, 1025) widened to float64 -> (B, length) float64."""
    assert re32.dtype == np.float32 and im32.dtype == np.float32
    return dsp.istft(re32.astype(np.float64), im32.astype(np.float64), length)


def large_istft_lengths():
    """The IH = 16 varlen case: 128 lengths drawn as tests/test_gpu_stft_lowpass.py::test_large_batch_bit_identical_per_clip draws
    them, with the two around the first sample the second group of 16 hops owns, and one of 14200 samples (33 frames: the row stride)."""
    rng = np.random.default_rng(7)
    lengths = [int(v) for v in rng.integers(1025, 14201, size=128)]
    lengths[5] = 14200
    edge = 16 * HOP - NFFT // 2
    lengths[40], lengths[41] = edge - 1, edge + 1
    return lengths


def f3_lengths():
    """The F = 3 varlen STFT case: 80 lengths in [1025, L65]; frame counts of every residue mod 3 (a wave's last group of three frames
    full, holding two frames, holding one), a clip of 1025 samples (3 frames: every later group of its row lies wholly past its end) and
    a clip of L65 samples (the row stride)."""
    rng = np.random.default_rng(11)
    lengths = [int(v) for v in rng.integers(1025, L65 + 1, size=80)]
    lengths[0] = 1025                       # 3 frames
    lengths[1] = L65                        # 65 frames = 2 mod 3
    lengths[2] = 30 * HOP - 1               # 30 frames = 0 mod 3
    lengths[3] = 30 * HOP                   # 31 frames = 1 mod 3
    lengths[4] = 31 * HOP + 200             # 32 frames = 2 mod 3
    return lengths


# ---------------------------------------------------------------------------------------------------------------------------------
# from_log and the energy match of unify_energy
# ---------------------------------------------------------------------------------------------------------------------------------
def from_log(x32):
    """10 ** min(x, 5) in float64 of float32 inputs (dsp.from_log states it in the input's own precision)."""
    assert np.asarray(x32).dtype == np.float32
    return dsp.from_log(np.asarray(x32, np.float64))


def from_log_inputs(B=3, T=65, seed=21):
    """(B, T, 128) float32 in [-9, 6.5]: uniform, with exactly 5.0, the float32 neighbours of 5.0, both ends of the range and integers
    (exact powers of ten) planted."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-9.0, 6.5, size=(B, T, NMEL)).astype(np.float32)
    flat = x.reshape(-1)
    plant = np.array([5.0, np.nextafter(np.float32(5.0), np.float32(6.0)), np.nextafter(np.float32(5.0), np.float32(4.0)), 6.5, -9.0,
                      0.0, 1.0, -1.0, 4.0, -8.0, 5.5], np.float32)
    at = rng.choice(flat.size, size=plant.size, replace=False)
    flat[at] = plant
    return x


def unify_inputs(B=3, T=65, lens_t=None, seed=31):
    """logmel (the estimate, as log10) and mel_in (the target, linear), (B, T, 128) float32, built so that a wrong band or frame limit
    shows: the two differ in spectral shape and in their course over time (opposite tilts over the bins and the frames), the bins 4
    and 25 just outside the band carry values at least 100 times their neighbours (the estimate's 100 x .. 200 x, the target's
    1000 x .. 2000 x: taking one in moves the ratio), and so does every frame at and past lens_t[b]."""
    rng = np.random.default_rng(seed)
    f = np.arange(NMEL)
    t = np.arange(T)[:, None]
    lg_est = rng.uniform(-2.0, -1.0, size=(B, T, NMEL)) + 0.02 * f + 0.008 * t      # rises by 2.5 decades over the bins, 0.5 over the frames
    lg_tgt = rng.uniform(-1.5, -0.5, size=(B, T, NMEL)) - 0.03 * f - 0.008 * t      # falls: no frame and no bin is typical of the sums
    for edge in (BAND_LO - 1, BAND_HI):
        near = [edge - 1, edge + 1]
        lg_est[:, :, edge] = lg_est[:, :, near].max(axis=2) + rng.uniform(2.0, 2.3, size=(B, T))
        lg_tgt[:, :, edge] = lg_tgt[:, :, near].max(axis=2) + rng.uniform(3.0, 3.3, size=(B, T))
    if lens_t is not None:
        for b, n in enumerate(lens_t):
            lg_est[b, n:] = lg_est[b, :n].max(axis=0) + rng.uniform(2.0, 2.3, size=(T - n, NMEL))     # per bin, over the clip's frames
            lg_tgt[b, n:] = lg_tgt[b, :n].max(axis=0) + rng.uniform(3.0, 3.3, size=(T - n, NMEL))
    assert lg_est.max() < 5.0       # the clamp of from_log stays out of this case
    return lg_est.astype(np.float32), (10.0 ** lg_tgt).astype(np.float32)


def unify_ratio(est32, mel_in32, lens_t=None, lo=BAND_LO, hi=BAND_HI, frame_shift=0):
    """sum(mel_in) / sum(est) over the bins lo .. hi - 1 and each clip's own frames, in float64 -> (B,).  est32: the float32 estimate
    10 ** min(logmel, 5) as the kernel itself produced it (the sums are the kernel's own values').  frame_shift: the frame limit moved
    by that many (the host test's off-by-one)."""
    est, tgt = np.asarray(est32, np.float64), np.asarray(mel_in32, np.float64)
    B, T, _ = est.shape
    out = np.empty(B)
    for b in range(B):
        n = (T if lens_t is None else lens_t[b]) + frame_shift
        out[b] = tgt[b, :n, lo:hi].sum() / est[b, :n, lo:hi].sum() if 0 < n <= T else np.nan
    return out


def unify_bound(n_frames):
    """|got / ref - 1| of an element of the scaled estimate: the two sums have n = 20 * frames positive terms each, so in ANY order of
    the float32 additions each carries at most (n - 1) roundings relative to itself; the quotient and the product add one each."""
    return (2 * 20 * n_frames + 2) * U32


# ---------------------------------------------------------------------------------------------------------------------------------
# vocoder input normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
def voc_tp(T):
    return T + T % 2 + 4


def voc_prep_inputs(B, T, seed=41, cfg=voc.VocoderConfig()):
    """(B, T, 128) float32 linear mel over twelve decades, both signs, with the branches of the map planted: exact zeros, values below
    amp_floor (after the band weight), values that clip at +R (20 log10 - 20 > 0: above 10 x the band weight)."""
    rng = np.random.default_rng(seed)
    w = voc.mel_band_weight(NMEL)
    x = (10.0 ** rng.uniform(-7.0, 1.5, size=(B, T, NMEL))) * rng.choice([-1.0, 1.0], size=(B, T, NMEL)) * w
    x[:, 0, :7] = 0.0
    x[:, 1, :] = 0.3 * cfg.amp_floor * w                   # below the floor
    x[:, 2, :] = -0.9 * cfg.amp_floor * w
    x[:, 3, :] = 50.0 * w                                  # clips at +R
    x[:, T - 1, 64:] = -1e3 * w[64:]
    return x.astype(np.float32)


def voc_prep_ref(mel32, Tp, lens_t=None, cfg=voc.VocoderConfig()):
    """oracle.vocoder.normalise_mel in float64 on each clip's own frames -> (B, Tp, 128); rows at and past them -R."""
    mel32 = np.asarray(mel32)
    assert mel32.dtype == np.float32
    B, T, _ = mel32.shape
    out = np.full((B, Tp, NMEL), -cfg.norm_range, np.float64)
    for b in range(B):
        n = T if lens_t is None else min(T, lens_t[b])
        if n:
            c = voc.normalise_mel(torch.from_numpy(mel32[b:b + 1, None, :n].astype(np.float64)), cfg)[0]     # (128, n + tail)
            out[b, :n] = c[:, :n].T.numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# peak normalisation + trim_center
# ---------------------------------------------------------------------------------------------------------------------------------
def peak_trim_ref(x32, L, peak, lens_l=None, lens_tp=None):
    """x32 (B, Llong) float32 -> (out (B, L) float64, divided (B,) bool).  Fixed form: the centre L samples, from (Llong - L) // 2.
    Varlen form: clip b = lens_l[b] samples of its lens_tp[b] * hop vocoder samples, from (lens_tp[b] * hop - lens_l[b]) // 2; zeros
    behind them.  A clip is divided by its peak where that exceeds 1."""
    x = np.asarray(x32)
    assert x.dtype == np.float32
    B, Llong = x.shape
    out = np.zeros((B, L), np.float64)
    divided = np.zeros(B, bool)
    for b in range(B):
        n = L if lens_l is None else lens_l[b]
        off = ((Llong if lens_l is None else lens_tp[b] * HOP) - n) // 2
        v = x[b, off:off + n].astype(np.float64)
        assert v.shape == (n,)
        p = float(np.float32(peak[b]))
        divided[b] = p > 1.0
        out[b, :n] = v / p if divided[b] else v
    return out, divided
