"""Splice restored clips onto their band-limited inputs: below a clip's cut-off bin the result is the input itself, above it the
restored clip, level-matched in the band just under the seam.  For bandwidth extension of clean, band-limited material, where the band
below the cut-off was fine to begin with and the network's copy of it (a new phase, a slightly different level) is the worse one.  Not
in the reference; its level half is amp_to_original_f (tools/utils.py:50-55).

All signals are at 44.1 kHz on the handle's front end (n_fft 2048, hop 441, periodic Hann, centred frames, reflect padding at the
clip's own ends, eps 1e-8).  Per clip, with x the input, y the restored clip, c the cut-off bin, w the ramp width in bins, g a gain:

    out = g y + ISTFT(a . STFT(x - g y)),    a = ramp_weights(c, w)

which by linearity is ISTFT(a STFT(x) + (1 - a) STFT(g y)) with one forward transform per frame, and leaves the band above the seam
as g y itself.  Engine.stft_splice evaluates it in one launch (csrc/stft.hip, k_stft_splice), Engine.band_power the two band powers
the gain is made of (csrc/splice.hip).  This module holds the rules in readable form and the list layer.
"""
import math

import numpy as np
import torch

from . import clips as _clips

N_BINS = 1025
HOP = 441
MIN_SAMPLES = 1025      # more than n_fft / 2 samples: the STFT's reflect padding
MAX_BATCH = 128         # clips per device call, as in the other list forms
SKIP_BINS = 5           # DC and the first bins never count in the level match, as amp_to_original_f skips [:5]


def ramp_weights(c, w):
    """The 1025 float32 weights of the input's spectrum: a[k] = 1 for k <= c - w - 1, 0 for k >= c, and float32(c - k) / float32(w + 1)
    -- one division -- between.  w = 0 is the hard mask of Engine.stft_lowpass."""
    c, w = int(c), int(w)
    if c < 0 or w < 0:
        raise ValueError("ramp_weights: need c >= 0 and w >= 0, got c=%d w=%d" % (c, w))
    k = np.arange(N_BINS, dtype=np.int64)
    a = (c - k).astype(np.float32) / np.float32(w + 1)
    a[k <= c - w - 1] = np.float32(1.0)
    a[k >= c] = np.float32(0.0)
    return a


def match_band(c, w, match=64):
    """The bins lo <= k < hi the level match compares: the `match` bins just under the ramp, never the first SKIP_BINS."""
    lo = max(SKIP_BINS, int(c) - int(w) - int(match))
    return lo, max(lo, int(c) - int(w))


def match_gain(p_in, p_out, n_terms, max_gain_db=12.0):
    """The gain that brings the restored clip's band power p_out to the input's p_in: sqrt(p_in / p_out) in float64 on the host,
    clamped to +-max_gain_db and rounded to float32.  1.0 for an empty band (n_terms == 0) and for a silent one: either power at or
    below 4e-8 * n_terms -- the eps clamp of the magnitude alone contributes 1e-8 per term."""
    p_in, p_out, n_terms = float(p_in), float(p_out), int(n_terms)
    floor = 4e-8 * n_terms
    if n_terms == 0 or not p_in > floor or not p_out > floor:
        return 1.0
    limit = 10.0 ** (float(max_gain_db) / 20.0)
    return float(np.float32(min(max(math.sqrt(p_in / p_out), 1.0 / limit), limit)))


def cut_bins_list(clips, threshold=0.95, engine=None):
    """The bandwidth detector's cut-off BIN of every clip of a list (Engine.band_energy's cut_bin at librosa's hop 512: the bins
    simulate.band_cutoff_list turns into Hz), in the caller's order; padded batches sorted by length, ONE device-to-host copy per batch.
    A clip too short for the reflect padding gets bin 0."""
    from . import simulate
    eng = simulate._engine_or_default(engine)
    lengths = [int(c.shape[0]) for c in clips]
    out = [0] * len(clips)
    for idx in _clips.batches([i for i in range(len(clips)) if lengths[i] >= MIN_SAMPLES], lengths, MAX_BATCH):
        x = _clips.pad([clips[i] for i in idx], eng.device, torch.float32)
        _, cut = eng.band_energy(x, lengths=[lengths[i] for i in idx], hop=simulate.BAND_HOP, threshold=threshold)
        for i, c in zip(idx, cut.cpu().tolist()):
            out[i] = int(c)
    return out


def splice_list(inputs, restored, cut_bins, ramp=8, match=64, max_gain_db=12.0, engine=None, to_host=False):
    """Splice every restored clip of a list onto its input -> (outs, gains) in the caller's order.  inputs, restored: 1-D clips (NumPy
    arrays or tensors, on any device), pair i of equal length (ValueError otherwise); cut_bins: one bin or one per clip; ramp: the
    width of the cross-fade in bins; match: the bins under the ramp whose power sets the gain of the restored clip (match_band,
    match_gain) -- 0: no level match, every gain is 1.  The pairs go to the device as float32 padded batches sorted by length, at
    most MAX_BATCH per call: one Engine.band_power call with ONE device-to-host copy of its (B, 2) block, then one Engine.stft_splice
    call.  A clip of at most 1024 samples (no reflect padding) or with cut-off bin 0 (nothing of the input to keep) is returned as
    its restored clip, gain 1.  outs: NumPy arrays (to_host) or device tensors."""
    from . import simulate
    inputs, restored = list(inputs), list(restored)
    if len(inputs) != len(restored):
        raise ValueError("splice_list: %d inputs and %d restored clips" % (len(inputs), len(restored)))
    n = len(inputs)
    cuts = [int(cut_bins)] * n if np.ndim(cut_bins) == 0 else [int(c) for c in cut_bins]
    if len(cuts) != n:
        raise ValueError("splice_list: %d cut-off bins for %d clips" % (len(cuts), n))
    lengths = []
    for i, (x, y) in enumerate(zip(inputs, restored)):
        if len(x.shape) != 1 or len(y.shape) != 1 or int(x.shape[0]) != int(y.shape[0]):
            raise ValueError("splice_list: clip %d: the input is %s and the restored clip %s (need two 1-D clips of one length)"
                             % (i, tuple(x.shape), tuple(y.shape)))
        if cuts[i] < 0:
            raise ValueError("splice_list: clip %d has cut-off bin %d (need >= 0)" % (i, cuts[i]))
        lengths.append(int(x.shape[0]))
    eng = simulate._engine_or_default(engine)
    outs, gains = [None] * n, [1.0] * n
    run = [i for i in range(n) if lengths[i] >= MIN_SAMPLES and cuts[i] > 0]
    for idx in _clips.batches(run, lengths, MAX_BATCH):
        lens = [lengths[i] for i in idx]
        x = _clips.pad([inputs[i] for i in idx], eng.device, torch.float32)
        y = _clips.pad([restored[i] for i in idx], eng.device, torch.float32)
        if match:
            # (a cut-off past the spectrum's last bin leaves a band of bins that do not exist: it ends where the spectrum does)
            bands = [tuple(min(k, N_BINS) for k in match_band(cuts[i], ramp, match)) for i in idx]
            power = eng.band_power(x, y, [b[0] for b in bands], [b[1] for b in bands], lengths=lens).cpu().tolist()    # the one copy
            for i, (lo, hi), (p_in, p_out) in zip(idx, bands, power):
                gains[i] = match_gain(p_in, p_out, (lengths[i] // HOP + 1) * (hi - lo), max_gain_db)
        out = eng.stft_splice(x, y, [cuts[i] for i in idx], lengths=lens, ramp=ramp, gains=[gains[i] for i in idx])
        for i, o in zip(idx, _clips.unpad(out, lens, to_host)):
            outs[i] = o
    for i in range(n):
        if outs[i] is None:
            outs[i] = _clips.as_numpy(restored[i]) if to_host else _clips.to_device(restored[i], eng.device)
    return outs, gains
