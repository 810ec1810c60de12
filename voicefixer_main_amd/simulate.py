"""Degradation simulator on the host side of the boundary.

The reference builds its training / test degradations from a handful of functions; the evaluation sets the handlers are run
on (`vctk_cheby1_1000`, `..._butter_...`, evaluation_proc/config.py:91-97) are produced with them.  Mirrored here with the
same names, argument meaning and error behaviour:

* ``lowpass(data, highcut, fs, order=5, _type="butter")``            tools/dsp/lowpass.py:152-187
    ``butter`` / ``cheby1`` / ``ellip`` / ``bessel``  -> ``lowpass_filter`` (zero-phase SOS filter)    :96-133
    ``stft``       -> ``stft_hard_lowpass``: polyphase resampling down to the cut-off rate and back up      :135-146
    ``stft_hard``  -> ``stft_hard_lowpass_v0``: STFT -> zero the bins above the cut-off -> ISTFT            :21-33
  (``_type in "butter"`` is a SUBSTRING test in the reference -- ``"b"``, ``"utt"`` and ``""`` all select the Butterworth
  filter; kept, since a config that relied on it must keep working);
* ``bandpass(data, lowcut, highcut, fs, order=5, _type="butter")``     tools/dsp/lowpass.py:189-215 (IIR types, same dispatch)
* ``band_cutoff(clip, fs, threshold)``: the bandwidth detector ``load_wav_energy`` of tools/utils.py:33-44 without the file read,
  in NumPy; ``band_cutoff_list`` is its batch form on the device (Engine.band_cutoff, csrc/band.hip);
* ``bandpass_filter`` / ``align_length`` / ``limit``                     tools/dsp/lowpass.py:35-94,148-150
* ``add_noise_and_scale`` / ``add_noise_and_scale_with_HQ`` / ``add_noise_and_scale_with_HQ_with_Aug``
                                                                           dataloaders/augmentation/base.py:33-118
  with their helpers ``normalize_energy`` / ``unify_energy`` (peak based: tools/others/audio_op.py:12-56); their ``..._list``
  forms mix whole lists of float32 clips on the device (Engine.mix_noise, csrc/mix.hip), ``hard_clip_list`` clips a list;
* ``reverb_rir(frames, rir)``                              dataloaders/augmentation/magical_effects.py:158-167
  (the `vctk_reverb` test set: convolution with a room impulse response; ``reverb_rir_list`` is its batch form on the device);
* ``quantification(samples, params)`` / ``time_dropout(frames, params)``   magical_effects.py:169-187, with ``smooth`` of
  tools/others/audio_op.py:152-174; ``quantification_list`` / ``time_dropout_list`` are their batch forms on the device
  (Engine.quantize, Engine.time_dropout, csrc/effects.hip);
* ``array_effects(frames, effects, rirs)``: the tail of ``MagicalEffects.effect`` behind the sox chain (:81-108) -- LARGESCALE,
  ``empty_c``, then reverb_rir, time_dropout and quant in dict order -- and ``array_effects_list``, whose clips stay on the device
  between steps; ``draw_array_effects`` draws the dicts as ``RandomServer.generate`` does (random_server.py:135-217);
* ``chain_effects(frames, effects)``: the sox chain in front of that tail (:41-64), as far as it is fully specified -- the biquads
  ``low_pass``, ``high_pass``, ``bass`` and ``treble`` (``biquad_design``), ``clip`` and ``reverse``, restated from published
  definitions and not pinned against sox --, ``magical_effects`` the whole of ``MagicalEffects.effect``, ``draw_effects`` the draws
  of every name; ``chain_effects_list`` / ``magical_effects_list`` are their batch forms on the device (Engine.effect_chain,
  csrc/chain.hip).  No device form, and no host form either: tempo, speed, pitch, fade, tremolo and reverb_freeverb.

Everything is NumPy / SciPy on the host EXCEPT ``stft_hard``: its STFT -> mask -> ISTFT round trip is the hot path's own
front-end and back-end (``vfx_stft_mel`` in its phase-emitting form and ``vfx_istft``), so it runs on the GPU through an
``Engine`` -- the reference keeps a module-level ``FDomainHelper`` for it (lowpass.py:14,111-113).  The list forms run it as
padded batches in one fused launch (``vfx_stft_lowpass``), bit for bit the single-clip form.
"""
import numpy as np
import torch

from . import clips as _clips

_engine = None     # the reference's module-level `f_helper` (lowpass.py:14): created on first use of `stft_hard`


def set_engine(engine):
    """Use this libvfx handle for `stft_hard` (otherwise one is created on cuda:0 at the first call)."""
    global _engine
    _engine = engine


def _get_engine():
    global _engine
    if _engine is None:
        from .engine import Engine
        _engine = Engine("cuda:0")
    return _engine


def _engine_or_default(engine):
    return engine if engine is not None else _get_engine()


# ------------------------------------------------------------------------------------------------------------------
# tools/dsp/lowpass.py
# ------------------------------------------------------------------------------------------------------------------
def align_length(x, y):
    """Length of y aligned to that of x: zero-padded at the end, or cut (lowpass.py:35-55)."""
    Lx, Ly = len(x), len(y)
    if Lx == Ly:
        return y
    if Lx > Ly:
        return np.pad(y, (0, Lx - Ly), mode="constant")
    return y[:Lx]


def limit(integer, high, low):
    """lowpass.py:148-150: clamp, and truncate to int inside the range."""
    if integer > high:
        return high
    if integer < low:
        return low
    return int(integer)


def _design(order, wn, btype, ftype, what):
    from scipy.signal import bessel, butter, cheby1, cheby2, ellip
    if ftype == "butter":
        return butter(order, wn, btype=btype, output="sos")
    if ftype == "cheby1":
        return cheby1(order, 0.1, wn, btype=btype, output="sos")
    if ftype == "cheby2":
        return cheby2(order, 60, wn, btype=btype, output="sos")
    if ftype == "ellip":
        return ellip(order, 0.1, 60, wn, btype=btype, output="sos")
    if ftype == "bessel":
        return bessel(order, wn, btype=btype, output="sos")
    raise Exception("The %s filter %s is not supported!" % (what, ftype))


def lowpass_filter(x, highcut, fs, order, ftype):
    """Zero-phase (forward-backward) IIR low-pass, second-order sections (lowpass.py:96-133): 0.1 dB ripple for cheby1 /
    ellip, 60 dB stop band for cheby2 / ellip."""
    from scipy.signal import sosfiltfilt
    sos = _design(order, highcut / (0.5 * fs), "low", ftype, "lowpass")
    y = sosfiltfilt(sos, x)
    return align_length(x, y) if len(y) != len(x) else y


def bandpass_filter(x, lowcut, highcut, fs, order, ftype):
    """lowpass.py:58-94."""
    from scipy.signal import sosfiltfilt
    nyq = 0.5 * fs
    sos = _design(order, [lowcut / nyq, highcut / nyq], "band", ftype, "bandpass")
    y = sosfiltfilt(sos, x)
    return align_length(x, y) if len(y) != len(x) else y


def stft_hard_lowpass(data, lowpass_ratio, fs_ori=44100):
    """`_type="stft"` (lowpass.py:135-146): polyphase resampling down to int(ratio * fs) and back up -- the band limit of a
    recording that really was sampled at the low rate."""
    from scipy.signal import resample_poly
    fs_down = int(lowpass_ratio * fs_ori)
    y = resample_poly(data, fs_down, fs_ori)
    y = resample_poly(y, fs_ori, fs_down)
    return align_length(data, y) if len(y) != len(data) else y


def stft_hard_lowpass_v0(data, lowpass_ratio, engine=None):
    """`_type="stft_hard"` (lowpass.py:21-33): |STFT|, cos, sin of the signal (eps = 1e-8: wav_to_spectrogram_phase), the
    magnitude bins from int(1025 * ratio) up set to zero, ISTFT to the original length.  Runs on the GPU: the front-end kernel
    in its phase-emitting form (`vfx_stft_mel`), the mask, `vfx_istft`.  Returns float32 (samples,) on the host like the
    reference's `.numpy()`."""
    eng = _engine_or_default(engine)
    length = data.shape[0]
    x = torch.as_tensor(np.ascontiguousarray(data), dtype=torch.float32)[None]
    o = eng.stft(x, want_mel=False, want_sp=True, want_phase=True)
    sp = o["sp"]
    cut = int(sp.shape[-1] * lowpass_ratio)
    sp[..., cut:] = 0.0
    return eng.istft(sp * o["cos"], sp * o["sin"], length)[0].cpu().numpy()


def _check_1d(clips):
    for data in clips:
        if len(list(data.shape)) != 1:
            raise ValueError("Error (chebyshev_lowpass_filter): Data " + str(data.shape) +
                             " should be type 1d time array, (samples,) , can not be (samples, 1)")


def _iir_type(_type, order):
    """The reference's substring tests for the IIR types, in its order, and its order clamp -> (name, order), or None."""
    for name in ("butter", "cheby1", "ellip", "bessel"):
        if _type in name:
            return name, limit(order, high=10, low=2)
    return None


def lowpass(data, highcut, fs, order=5, _type="butter", engine=None):
    """lowpass.py:152-187.  data: 1-D float array (samples,) -- (samples, 1) is an error, as in the reference."""
    _check_1d([data])
    iir = _iir_type(_type, order)
    if iir:
        return lowpass_filter(x=data, highcut=int(highcut), fs=fs, order=iir[1], ftype=iir[0])
    if _type in "stft":
        return stft_hard_lowpass(data, lowpass_ratio=highcut / int(fs / 2))
    if _type in "stft_hard":
        return stft_hard_lowpass_v0(data, lowpass_ratio=highcut / int(fs / 2), engine=engine)
    raise ValueError("Error: Unexpected filter type " + _type)


def bandpass(data, lowcut, highcut, fs, order=5, _type="butter"):
    """lowpass.py:189-215: the band-pass twin of `lowpass` -- same 1-D check, same substring dispatch and order clamp, IIR
    types only (butter / cheby1 / ellip / bessel; cheby2 is commented out in the reference and raises here as well)."""
    _check_1d([data])
    iir = _iir_type(_type, order)
    if iir:
        return bandpass_filter(x=data, lowcut=int(lowcut), highcut=int(highcut), fs=fs, order=iir[1], ftype=iir[0])
    raise ValueError("Error: Unexpected filter type " + _type)


# ------------------------------------------------------------------------------------------------------------------
# batch forms: a whole test set of clips per call, the IIR types on the device (Engine.sosfiltfilt, csrc/sosfilt.hip).
# Ordering by length, batching, padding and handing the rows back are clips.py's; a function here decides which items go to
# the device, what a batch is made of and which Engine method takes it.
# ------------------------------------------------------------------------------------------------------------------
MAX_BATCH = 128     # clips per device call, as in restore_list / evaluation_list


def _sosfiltfilt_list(clips, sos, engine, to_host):
    """scipy.signal.sosfiltfilt(sos, clip) of every clip, in padded batches of one dtype (float32 clips are extended in float32, as
    SciPy does; every other dtype goes as float64), results in the caller's order."""
    eng = _engine_or_default(engine)
    padlen = eng.sosfiltfilt_padlen(sos)
    if any(c.shape[0] <= padlen for c in clips):
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    lengths = [c.shape[0] for c in clips]
    out = [None] * len(clips)
    for f32 in (True, False):
        dtype = torch.float32 if f32 else torch.float64
        for idx in _clips.batches([i for i in range(len(clips)) if _clips.is_f32(clips[i]) == f32], lengths, MAX_BATCH):
            lens = [lengths[i] for i in idx]
            y = eng.sosfiltfilt(_clips.pad([clips[i] for i in idx], eng.device, dtype), sos, lengths=lens)
            for i, row in zip(idx, _clips.unpad(y, lens, to_host)):
                out[i] = row
    return out


def _stft_group(clips, ratio, eng, to_host, fs_ori):
    """`_stft_list` for clips of ONE ratio on an engine without `resample_each`: float32 clips whose two rate pairs `Engine.resample`
    takes go down and up through it as padded batches; everything else is left to the host (None)."""
    from .engine import Engine
    fs_down = int(ratio * fs_ori)
    on_device = fs_down > 0 and fs_down != fs_ori and Engine.resample_supported(fs_ori, fs_down) and Engine.resample_supported(fs_down, fs_ori)
    lengths = [c.shape[0] for c in clips]
    out = [None] * len(clips)
    dev = [i for i in range(len(clips)) if on_device and _clips.is_f32(clips[i]) and lengths[i] > 0]
    for idx in _clips.batches(dev, lengths, MAX_BATCH):
        lens = [lengths[i] for i in idx]
        low, low_lengths = eng.resample(_clips.pad([clips[i] for i in idx], eng.device, torch.float32), fs_ori, fs_down, lengths=lens)
        y, _ = eng.resample(low, fs_down, fs_ori, lengths=low_lengths)
        if y.shape[1] < lens[-1]:      # align_length: cut, or zero-padded at the end (rows are zero past their length)
            y = torch.nn.functional.pad(y, (0, lens[-1] - y.shape[1]))
        for i, row in zip(idx, _clips.unpad(y, lens, to_host)):
            out[i] = row
    return out


def _stft_list(clips, ratios, engine, to_host, fs_ori=44100):
    """`_type="stft"` for a list, ratios[i] the ratio of clip i: bit for bit `stft_hard_lowpass`, item by item.  Non-empty float32 and
    float64 items (device tensors included, as they are) with 0 < fs_down != fs_ori and a rate pair Engine.resample_each takes are
    grouped by dtype, sorted by length and cut into batches of MAX_BATCH whatever their cut-offs; a batch costs TWO calls: down with
    a rate per clip, up with n_out = the batch's longest clip, which is `align_length`'s cut or zero pad (rows are zero past their
    output length).  Everything else -- other dtypes, empty clips, fs_down <= 0, fs_down == fs_ori, a pair past the cap -- takes the
    host function.  An engine without `resample_each` keeps the older path: per distinct ratio, float32 clips at the pairs
    Engine.resample takes go through it, the rest to the host."""
    eng = _engine_or_default(engine)
    lengths = [c.shape[0] for c in clips]
    out = [None] * len(clips)
    if hasattr(eng, "resample_each"):
        from .engine import Engine
        downs = [int(r * fs_ori) for r in ratios]
        takes = {d: 0 < d != fs_ori and Engine.resample_each_supported(fs_ori, d) and Engine.resample_each_supported(d, fs_ori)
                 for d in set(downs)}
        for dtype in (torch.float32, torch.float64):
            name = str(dtype).split(".")[-1]
            dev = [i for i in range(len(clips)) if str(clips[i].dtype).endswith(name) and lengths[i] > 0 and takes[downs[i]]]
            for idx in _clips.batches(dev, lengths, MAX_BATCH):
                lens = [lengths[i] for i in idx]
                rates = [downs[i] for i in idx]
                low, low_lengths = eng.resample_each(_clips.pad([clips[i] for i in idx], eng.device, dtype), fs_ori, rates, lengths=lens)
                y, _ = eng.resample_each(low, rates, fs_ori, lengths=low_lengths, n_out=lens[-1])
                for i, row in zip(idx, _clips.unpad(y, lens, to_host)):
                    out[i] = row
    else:
        groups = {}
        for i, r in enumerate(ratios):
            groups.setdefault(r, []).append(i)
        for r, idx in groups.items():
            for i, y in zip(idx, _stft_group([clips[i] for i in idx], r, eng, to_host, fs_ori)):
                out[i] = y
    for i in range(len(clips)):
        if out[i] is None:
            y = stft_hard_lowpass(_clips.as_numpy(clips[i]), lowpass_ratio=ratios[i], fs_ori=fs_ori)
            out[i] = y if to_host else _clips.to_device(y, eng.device)
    return out


def _stft_hard_list(clips, ratios, engine, to_host):
    """`_type="stft_hard"` for a list, ratios[i] the ratio of clip i: every clip as float32 (what `stft_hard_lowpass_v0` makes of any
    dtype), cut = int(1025 * ratio) as there, sorted by length and through Engine.stft_lowpass as padded batches of up to MAX_BATCH --
    ONE launch per batch, each clip bit for bit its own `stft_hard_lowpass_v0` call.  An item of at most 1024 samples (no reflect
    padding) or with a negative cut, and every item of an engine without `stft_lowpass`, takes that function, and raises what it
    raises."""
    eng = _engine_or_default(engine)
    lengths = [c.shape[0] for c in clips]
    cuts = [int(1025 * r) for r in ratios]
    out = [None] * len(clips)
    dev = [i for i in range(len(clips)) if hasattr(eng, "stft_lowpass") and lengths[i] > 1024 and cuts[i] >= 0]
    for idx in _clips.batches(dev, lengths, MAX_BATCH):
        lens = [lengths[i] for i in idx]
        y = eng.stft_lowpass(_clips.pad([clips[i] for i in idx], eng.device, torch.float32), [cuts[i] for i in idx], lengths=lens)
        for i, row in zip(idx, _clips.unpad(y, lens, to_host)):
            out[i] = row
    for i in range(len(clips)):
        if out[i] is None:
            y = stft_hard_lowpass_v0(_clips.as_numpy(clips[i]), lowpass_ratio=ratios[i], engine=eng)
            out[i] = y if to_host else _clips.to_device(y, eng.device)
    return out


def lowpass_list(clips, highcut, fs, order=5, _type="butter", engine=None, to_host=True):
    """`lowpass` for a list of 1-D clips of any lengths: the same 1-D check, substring dispatch, int() of the cut-off and order
    clamp, ONE filter design, and the IIR types as padded batches on the device -- every clip bit for bit what
    scipy.signal.sosfiltfilt gives for it alone; "stft_hard" as padded batches through Engine.stft_lowpass, every clip bit for bit
    `stft_hard_lowpass_v0`.  -> list in the caller's order: float64 NumPy arrays (to_host), or device tensors
    that `restore_list` takes as they are."""
    clips = list(clips)
    _check_1d(clips)
    iir = _iir_type(_type, order)
    if iir:
        return _sosfiltfilt_list(clips, _design(iir[1], int(highcut) / (0.5 * fs), "low", iir[0], "lowpass"), engine, to_host)
    if _type in "stft":
        return _stft_list(clips, [highcut / int(fs / 2)] * len(clips), engine, to_host)
    if _type in "stft_hard":
        return _stft_hard_list(clips, [highcut / int(fs / 2)] * len(clips), engine, to_host)
    raise ValueError("Error: Unexpected filter type " + _type)


def bandpass_list(clips, lowcut, highcut, fs, order=5, _type="butter", engine=None, to_host=True):
    """`bandpass` for a list of 1-D clips, as `lowpass_list` (IIR types only)."""
    clips = list(clips)
    _check_1d(clips)
    iir = _iir_type(_type, order)
    if iir:
        nyq = 0.5 * fs
        sos = _design(iir[1], [int(lowcut) / nyq, int(highcut) / nyq], "band", iir[0], "bandpass")
        return _sosfiltfilt_list(clips, sos, engine, to_host)
    raise ValueError("Error: Unexpected filter type " + _type)


# ------------------------------------------------------------------------------------------------------------------
# a filter per clip: what the training collator draws (dataloaders/data_module.py:14-70).  The IIR items of a call share
# Engine.sosfiltfilt_bank launches whatever their designs (csrc/sosfilt.hip, k_sosfilt_bank).
# ------------------------------------------------------------------------------------------------------------------
def _per_clip(value, n, name):
    """A scalar, or a sequence with one entry per clip -> list of n."""
    if isinstance(value, str) or np.ndim(value) == 0:
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError("%s: %d entries for %d clips" % (name, len(value), n))
    return value


def _sosfiltfilt_each(clips, design_of, designs, engine, to_host):
    """scipy.signal.sosfiltfilt(designs[design_of[i]], clips[i]) for every i of the dict `design_of`, batched by dtype and length
    as `_sosfiltfilt_list` does; a batch's bank is the designs it uses.  -> {i: result}"""
    eng = _engine_or_default(engine)
    padlens = [eng.sosfiltfilt_padlen(sos) for sos in designs]
    for i, d in design_of.items():
        if clips[i].shape[0] <= padlens[d]:
            raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlens[d])
    lengths = [c.shape[0] for c in clips]
    out = {}
    for f32 in (True, False):
        dtype = torch.float32 if f32 else torch.float64
        for idx in _clips.batches([i for i in design_of if _clips.is_f32(clips[i]) == f32], lengths, MAX_BATCH):
            lens = [lengths[i] for i in idx]
            used = sorted({design_of[i] for i in idx})
            y = eng.sosfiltfilt_bank(_clips.pad([clips[i] for i in idx], eng.device, dtype), [designs[d] for d in used],
                                     filter_index=[used.index(design_of[i]) for i in idx], lengths=lens)
            out.update(zip(idx, _clips.unpad(y, lens, to_host)))
    return out


def _filter_each(clips, cuts, fs, orders, types, engine, to_host):
    """cuts[i]: (highcut,) -- `lowpass` -- or (lowcut, highcut) -- `bandpass` -- of clip i.  Every item is sorted to its path first,
    so an error is raised before anything runs."""
    _check_1d(clips)
    band = len(cuts[0]) == 2 if cuts else False
    nyq = 0.5 * fs
    designs, keys, design_of, stft, hard = [], {}, {}, [], []
    for i, (cut, order, _type) in enumerate(zip(cuts, orders, types)):
        iir = _iir_type(_type, order)
        if iir:
            key = (iir[0], iir[1]) + tuple(int(v) for v in cut)
            if key not in keys:      # one design per distinct (name, order, cut-offs)
                wn = [v / nyq for v in key[2:]]
                keys[key] = len(designs)
                designs.append(_design(iir[1], wn if band else wn[0], "band" if band else "low", iir[0], "bandpass" if band else "lowpass"))
            design_of[i] = keys[key]
        elif not band and _type in "stft":
            stft.append(i)
        elif not band and _type in "stft_hard":
            hard.append(i)
        else:
            raise ValueError("Error: Unexpected filter type " + _type)
    out = [None] * len(clips)
    if design_of:
        for i, y in _sosfiltfilt_each(clips, design_of, designs, engine, to_host).items():
            out[i] = y
    if stft:      # one list whatever the cut-offs: a ratio per clip
        for i, y in zip(stft, _stft_list([clips[i] for i in stft], [cuts[i][0] / int(fs / 2) for i in stft], engine, to_host)):
            out[i] = y
    if hard:
        ys = _stft_hard_list([clips[i] for i in hard], [cuts[i][0] / int(fs / 2) for i in hard], engine, to_host)
        for i, y in zip(hard, ys):
            out[i] = y
    return out


def lowpass_each(clips, highcuts, fs, orders=5, types="butter", engine=None, to_host=True):
    """`lowpass(clips[i], highcuts[i], fs, orders[i], types[i])` for every clip of a list -- exactly that function's result,
    item by item, in the caller's order.  `highcuts`, `orders` and `types` are each a scalar or a sequence with one entry per clip;
    per clip the 1-D check, the substring dispatch, int() of the cut-off and the order clamp are `lowpass`'s.  The IIR items are
    designed once per distinct (name, order, cut-off) and go through Engine.sosfiltfilt_bank as padded batches of one dtype, ONE
    launch pair per batch whatever its designs; "stft" items go through Engine.resample_each as padded batches with a rate pair per
    clip, two calls per batch whatever its cut-offs (`_stft_list`'s rule for which items), "stft_hard" items through
    Engine.stft_lowpass as padded batches with a cut-off bin per clip (`_stft_hard_list`).
    -> list: NumPy arrays (to_host), or device tensors."""
    clips = list(clips)
    n = len(clips)
    highcuts = _per_clip(highcuts, n, "lowpass_each: highcuts")
    return _filter_each(clips, [(h,) for h in highcuts], fs, _per_clip(orders, n, "lowpass_each: orders"),
                        _per_clip(types, n, "lowpass_each: types"), engine, to_host)


def bandpass_each(clips, lowcuts, highcuts, fs, orders=5, types="butter", engine=None, to_host=True):
    """`bandpass(clips[i], lowcuts[i], highcuts[i], fs, orders[i], types[i])` for every clip of a list, as `lowpass_each` (IIR
    types only)."""
    clips = list(clips)
    n = len(clips)
    cuts = list(zip(_per_clip(lowcuts, n, "bandpass_each: lowcuts"), _per_clip(highcuts, n, "bandpass_each: highcuts")))
    return _filter_each(clips, cuts, fs, _per_clip(orders, n, "bandpass_each: orders"), _per_clip(types, n, "bandpass_each: types"),
                        engine, to_host)


# ------------------------------------------------------------------------------------------------------------------
# the bandwidth detector in front of the restoration handlers (tools/utils.py:33-44 load_wav_energy; eval_ssr_unet.py:105-106 pairs it
# with lowpass(..., _type="stft")): the frequency below which `threshold` of a clip's log-spectral energy lies
# ------------------------------------------------------------------------------------------------------------------
BAND_NFFT, BAND_HOP, BAND_BINS = 2048, 512, 1025     # librosa.stft's defaults


def band_cutoff_hz(cut_bin, fs):
    """The reference's last expression (utils.py:44): bin -> Hz."""
    return int((int(fs) // 2) * (cut_bin / BAND_BINS))


def band_cutoff(clip, fs=44100, threshold=0.95):
    """load_wav_energy's cut-off in Hz of ONE clip (samples,), on the host in NumPy with the reference's number formats: librosa.stft's
    defaults (n_fft 2048, hop 512, periodic Hann, centred, reflect padding; the transform in float64, stored as complex64), float32
    magnitudes, logarithms and sums.  e[k] = sum_t log10(|S[k, t]| + 1); P[k] = sum(e[:k]), the exclusive prefix the loop of
    utils.py:38-39 leaves (it runs from the top down, so every sum sees original values); total = P[1024]; the cut-off bin is the
    first k that does not have P[k] < total * threshold."""
    x = np.asarray(_clips.as_numpy(clip), dtype=np.float32).reshape(-1)
    xp = np.pad(x, BAND_NFFT // 2, mode="reflect")
    idx = np.arange(x.shape[0] // BAND_HOP + 1)[:, None] * BAND_HOP + np.arange(BAND_NFFT)[None, :]
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(BAND_NFFT) / BAND_NFFT)
    spec = np.fft.rfft(xp[idx] * window, axis=-1).astype(np.complex64).T          # (1025, T)
    e = np.sum(np.log10(np.abs(spec) + 1.0), axis=1)
    prefix = np.array([np.sum(e[:k]) for k in range(e.shape[0])], dtype=e.dtype)
    level = prefix[-1] * threshold
    cut_bin = e.shape[0] - 1
    for k in range(e.shape[0]):
        if not prefix[k] < level:
            cut_bin = k
            break
    return band_cutoff_hz(cut_bin, fs)


def band_cutoff_list(clips, fs=44100, threshold=0.95, engine=None):
    """`band_cutoff` for a list of 1-D clips of any lengths (NumPy arrays or tensors, on any device) -> [Hz per clip] in the caller's
    order.  Clips of more than 1024 samples go through Engine.band_cutoff as float32 padded batches, sorted by length, up to MAX_BATCH
    per call, ONE device-to-host copy per batch; a clip's cut-off does not depend on its batch.  The device sums in float64 where the
    host form sums in float32: the two agree wherever the decision is not within rounding of a bin's edge.  Shorter clips take the
    host form."""
    clips = list(clips)
    _check_1d(clips)
    eng = _engine_or_default(engine)
    lengths = [c.shape[0] for c in clips]
    out = [None] * len(clips)
    for idx in _clips.batches([i for i in range(len(clips)) if lengths[i] > BAND_NFFT // 2], lengths, MAX_BATCH):
        lens = [lengths[i] for i in idx]
        x = _clips.pad([clips[i] for i in idx], eng.device, torch.float32)
        for i, hz in zip(idx, eng.band_cutoff(x, lengths=lens, sample_rate=fs, hop=BAND_HOP, threshold=threshold)):
            out[i] = hz
    for i in range(len(clips)):
        if out[i] is None:
            out[i] = band_cutoff(clips[i], fs, threshold)
    return out


def draw_lowpass_params(n, low_pass_range, filter_order_range, filter_type, rng):
    """The training collator's three draws per item, in its order (data_module.py:28-33): the cut-off int(U(lo // 2, hi // 2)), the
    order int(U(o_lo, o_hi)), the type filter_type[int(U(0, len))].  -> (cutoffs, orders, filters), n entries each."""
    cutoffs, orders, filters = [], [], []
    for _ in range(n):
        cutoffs.append(int(_uniform(int(low_pass_range[0] // 2), int(low_pass_range[1] // 2), rng)))
        orders.append(int(_uniform(filter_order_range[0], filter_order_range[1], rng)))
        filters.append(filter_type[int(_uniform(0, len(filter_type), rng))])
    return cutoffs, orders, filters


def lowpass_collate(batch, low_pass_range, filter_order_range, filter_type, fs, rng=None, engine=None, to_host=False):
    """LowpassTrainCollator.__call__ (data_module.py:28-70) for a batch of dicts of (L, C) arrays: per item a cut-off, an order and
    a type from `draw_lowpass_params`; `fname` keys pass through as lists; every other key is stacked as (B, L, 1) float32 from
    channel 0.  For a key containing "vocals", then for one containing "noise", one chance = U(0, 1000) is drawn per item in item
    order: vocals are always low-passed with the item's type, and again with "stft" when int(chance) is even; noise stays as it is
    when int(chance) is even, otherwise it is low-passed with the item's type, and again with "stft" when int(chance) % 3 == 0.
    All items of a key share ONE `lowpass_each` call, the "stft" follow-ups a second one; key + "_LR" is the (B, L, 1) float32
    stack, every item exactly what the single-clip `lowpass` chain gives, rounded to float32.  -> dict of tensors on the engine's
    device, or on the host (to_host).  Items of unequal length raise ValueError (the reference's torch.stack raises).  An
    untouched noise item contributes its channel 0 (the reference stacks the whole (L, C) array, which only stacks with filtered
    items when C = 1).  NOT mirrored: the reference's early return for an empty low_pass_range (lines 23-26) reads `ret[key]`
    from an empty dict and can only raise; here such a range draws its one cut-off, as `_uniform` gives it."""
    rng = rng if rng is not None else np.random.default_rng()
    batch = list(batch)
    cutoffs, orders, filters = draw_lowpass_params(len(batch), low_pass_range, filter_order_range, filter_type, rng)
    eng = _engine_or_default(engine)
    where = torch.device("cpu") if to_host else eng.device

    def stack(key, rows):
        if len({r.shape[0] for r in rows}) > 1:
            raise ValueError("lowpass_collate: %s: items of %s samples do not stack" % (key, sorted({r.shape[0] for r in rows})))
        return torch.stack([_clips.as_tensor(r).to(device=where, dtype=torch.float32) for r in rows])[..., None]

    def each(rows, idx, types):      # rows[i] <- lowpass of rows[i], i in idx
        pick = lambda v: [v[i] for i in idx]      # noqa: E731
        ys = lowpass_each(pick(rows), pick(cutoffs), fs, pick(orders), types, engine=eng, to_host=to_host)
        for i, y in zip(idx, ys):
            rows[i] = y

    ret = {}
    for key in (batch[0].keys() if batch else ()):
        if "fname" in key:
            ret[key] = [x[key] for x in batch]
            continue
        clips = [x[key][..., 0] for x in batch]
        ret[key] = stack(key, clips)
        for word in ("vocals", "noise"):
            if word not in key:
                continue
            chances = [int(_uniform(0, 1000, rng)) for _ in batch]
            if word == "vocals":
                first = list(range(len(batch)))
                again = [i for i in first if chances[i] % 2 == 0]
            else:
                first = [i for i in range(len(batch)) if chances[i] % 2 != 0]
                again = [i for i in first if chances[i] % 3 == 0]
            rows = list(clips)
            each(rows, first, [filters[i] for i in first])
            each(rows, again, "stft")
            ret[key + "_LR"] = stack(key + "_LR", rows)
    return ret


VAL_CUTOFFS = (1000, 2000, 4000, 8000, 12000)


def lowpass_collate_val(batch, engine=None, to_host=False):
    """collate_fn_val (data_module.py:130-150) for a batch of dicts of (L, C) arrays: `fname` keys pass through as lists; every other
    key is stacked as (B, L, 1) float32 from channel 0, and for every c in VAL_CUTOFFS key + "LR_" + str(c) is the (B, L, 1) float32
    stack of lowpass(lowpass(x, c, 44100, 8, "butter"), c, 44100, 8, "stft") -- one `lowpass_list` call per filter, cut-off and key,
    the "stft" pass on the float64 device rows of the Butterworth pass; every item exactly what the single-clip chain gives, rounded
    to float32.  "cutoffs_c" / "orders_c" / "filters_c" are kept as the reference fills them: the list of cut-offs and two empty
    lists.  -> tensors on the engine's device, or on the host (to_host)."""
    batch = list(batch)
    eng = _engine_or_default(engine)
    where = torch.device("cpu") if to_host else eng.device

    def stack(rows):
        return torch.stack([_clips.as_tensor(r).to(device=where, dtype=torch.float32) for r in rows])[..., None]

    ret = {}
    for key in (batch[0].keys() if batch else ()):
        if "fname" in key:
            ret[key] = [x[key] for x in batch]
            continue
        clips = [x[key][..., 0] for x in batch]
        ret[key] = stack(clips)
        for c in VAL_CUTOFFS:
            rows = lowpass_list(clips, c, 44100, order=8, _type="butter", engine=eng, to_host=to_host)
            rows = lowpass_list(rows, c, 44100, order=8, _type="stft", engine=eng, to_host=to_host)
            ret[key + "LR_" + str(c)] = stack(rows)
            ret["cutoffs_" + str(c)] = list(VAL_CUTOFFS)
            ret["orders_" + str(c)] = []
            ret["filters_" + str(c)] = []
    return ret


# ------------------------------------------------------------------------------------------------------------------
# dataloaders/augmentation/magical_effects.py:158-167
# ------------------------------------------------------------------------------------------------------------------
def reverb_rir(frames, rir):
    """MagicalEffects.reverb_rir: both inputs squeezed, convolved over the full length, the whole result scaled to a peak of 0.98
    when its peak exceeds 0.99, cut to the first frames.shape[0] samples."""
    from scipy.signal import convolve
    orig_frames_shape = frames.shape
    frames, filt = np.squeeze(frames), np.squeeze(rir)
    frames = convolve(frames, filt)
    actlev = np.max(np.abs(frames))
    if actlev > 0.99:
        frames = (frames / actlev) * 0.98
    return frames[:orig_frames_shape[0]]


def reverb_rir_list(clips, rirs, rir_index=None, engine=None, to_host=True):
    """`reverb_rir` for a list of clips and a list of RIRs (or one RIR): clip i takes RIR rir_index[i] (default i % len(rirs)).
    float32 clips with float32 RIRs are sorted by length and go through Engine.reverb_rir as padded batches of up to MAX_BATCH --
    direct-form convolution, each clip bit for bit what its own device call gives; every other dtype takes the host function.
    -> list in the caller's order: NumPy arrays (to_host), or device tensors that `restore_list` takes as they are."""
    clips = list(clips)
    rirs = [rirs] if isinstance(rirs, (np.ndarray, torch.Tensor)) else list(rirs)
    if not rirs:
        raise ValueError("reverb_rir_list: no RIR")
    rir_index = [i % len(rirs) for i in range(len(clips))] if rir_index is None else [int(v) for v in rir_index]
    if len(rir_index) != len(clips) or any(not 0 <= r < len(rirs) for r in rir_index):
        raise ValueError("reverb_rir_list: %d indices for %d clips, each must be in [0, %d)" % (len(rir_index), len(clips), len(rirs)))
    eng = _engine_or_default(engine)

    def flat(a):     # the 1-D tensor form of a clip or RIR that np.squeeze makes 1-D and non-empty, or None
        t = _clips.as_tensor(a).squeeze()
        return t if t.dim() == 1 and t.numel() > 0 else None

    def on_device(clip, rir):      # (a clip that squeezes to another length than shape[0] is cut differently: host)
        c, r = flat(clip), flat(rir)
        return (_clips.is_f32(clip) and _clips.is_f32(rir) and c is not None and r is not None and c.numel() == clip.shape[0]
                and r.numel() <= eng.MAX_RIR_TAPS)

    lengths = [c.shape[0] for c in clips]
    out = [None] * len(clips)
    dev = [i for i in range(len(clips)) if on_device(clips[i], rirs[rir_index[i]])]
    for idx in _clips.batches(dev, lengths, MAX_BATCH):
        lens = [lengths[i] for i in idx]
        used = sorted({rir_index[i] for i in idx})      # the batch's bank: the RIRs it uses, padded like the clips
        taps = [flat(rirs[r]) for r in used]
        y, _ = eng.reverb_rir(_clips.pad([flat(clips[i]) for i in idx], eng.device, torch.float32),
                              _clips.pad(taps, eng.device, torch.float32), rir_index=[used.index(rir_index[i]) for i in idx],
                              lengths=lens, rir_lengths=[t.numel() for t in taps])
        for i, row in zip(idx, _clips.unpad(y, lens, to_host)):
            out[i] = row
    for i in range(len(clips)):
        if out[i] is None:
            y = reverb_rir(_clips.as_numpy(clips[i]), _clips.as_numpy(rirs[rir_index[i]]))
            out[i] = y if to_host else _clips.to_device(y, eng.device)
    return out


# ------------------------------------------------------------------------------------------------------------------
# tools/others/audio_op.py:12-56 (peak-based "energy") and dataloaders/augmentation/base.py:33-118
# ------------------------------------------------------------------------------------------------------------------
def activelev(*args):
    """Largest absolute sample over all the signals (audio_op.py:41-56)."""
    return max(float(np.max(np.abs(np.asarray(a)))) for a in args)


def normalize_energy(audio, alpha=1):
    """Peak to alpha (audio_op.py:12-29)."""
    return (audio / activelev(audio)) * alpha


def unify_energy(*args):
    """All signals by ONE factor so that the largest peak among them becomes 1 (audio_op.py:31-39)."""
    s = 1.0 / activelev(*args)
    return [x * s for x in args]


def _uniform(lower, upper, rng):
    """tools/pytorch/random_.py:28-31: the upper bound itself when the interval is (almost) empty."""
    if abs(lower - upper) < 1e-5:
        return upper
    return float((upper - lower) * rng.random() + lower)


def _random_noise(clean, noise, snr_l, snr_h, rng):
    """base.py:112-115: the NOISE is divided by 10 ** (snr / 20), snr ~ U[snr_l, snr_h) dB."""
    snr = _uniform(snr_l, snr_h, rng)
    return clean, noise / (10 ** (float(snr) / 20)), snr


def add_noise_and_scale(front, noise, snr_l=-5, snr_h=35, scale_lower=0.6, scale_upper=1.0, rng=None):
    """base.py:33-54: both signals to unit peak, the noise lowered by a random SNR (peak ratio, dB), the mixture's peak
    to 1 (all three by the same factor), a random common scale.  -> (front, noise, snr, scale); noisy = front + noise."""
    rng = rng if rng is not None else np.random.default_rng()
    snr = None
    noise, front = normalize_energy(noise), normalize_energy(front)
    if snr_l is not None and snr_h is not None:
        front, noise, snr = _random_noise(front, noise, snr_l, snr_h, rng)
    _, noise, front = unify_energy(noise + front, noise, front)
    scale = _uniform(scale_lower, scale_upper, rng)
    return front * scale, noise * scale, snr, scale


def _match_noise_level(noise, level_of):
    """base.py:74-78 / :101-105: "some clipping noise is extremely noisy" -- unless the speech is nearly silent, the noise's
    mean absolute level is set to the speech's before the SNR is applied."""
    front_level = float(np.mean(np.abs(level_of)))
    if front_level > 0.02:
        noise = noise / (float(np.mean(np.abs(noise))) / front_level)
    return noise


def add_noise_and_scale_with_HQ(HQ, front, noise, snr_l=-5, snr_h=35, scale_lower=0.6, scale_upper=1.0, rng=None):
    """base.py:86-110 -> (HQ, front, noise, snr, scale)."""
    rng = rng if rng is not None else np.random.default_rng()
    snr = None
    noise = normalize_energy(noise)
    HQ, front = unify_energy(HQ, front)
    noise = _match_noise_level(noise, front)
    if snr_l is not None and snr_h is not None:
        front, noise, snr = _random_noise(front, noise, snr_l, snr_h, rng)
    _, noise, front, HQ = unify_energy(noise + front, noise, front, HQ)
    scale = _uniform(scale_lower, scale_upper, rng)
    return HQ * scale, front * scale, noise * scale, snr, scale


def add_noise_and_scale_with_HQ_with_Aug(HQ, front, augfront, noise, snr_l=-5, snr_h=35, scale_lower=0.6, scale_upper=1.0,
                                         rng=None):
    """base.py:56-84 -> (HQ, front, augfront, noise, snr, scale); the noise is mixed into the AUGMENTED speech."""
    rng = rng if rng is not None else np.random.default_rng()
    snr = None
    noise = normalize_energy(noise)
    HQ, front, augfront = unify_energy(HQ, front, augfront)
    noise = _match_noise_level(noise, augfront)
    if snr_l is not None and snr_h is not None:
        augfront, noise, snr = _random_noise(augfront, noise, snr_l, snr_h, rng)
    _, augfront, noise, front, HQ = unify_energy(noise + augfront, augfront, noise, front, HQ)
    scale = _uniform(scale_lower, scale_upper, rng)
    return HQ * scale, front * scale, augfront * scale, noise * scale, snr, scale


def hard_clip(x, threshold):
    """The declipping test sets' degradation: samples limited to +-threshold (config/vctk_base_voicefixer_unet.json:80-100)."""
    return np.clip(x, -threshold, threshold)


# ------------------------------------------------------------------------------------------------------------------
# batch forms of the noise mixers (Engine.mix_noise, csrc/mix.hip) and of hard_clip
# ------------------------------------------------------------------------------------------------------------------
_MIX_FORMS = (     # the host function and its signals in argument order (= the order it returns them in)
    (add_noise_and_scale, ("front", "noise")),
    (add_noise_and_scale_with_HQ, ("hq", "front", "noise")),
    (add_noise_and_scale_with_HQ_with_Aug, ("hq", "front", "aug", "noise")),
)


def _mix_list(form, signals, snr_l, snr_h, scale_lower, scale_upper, rng, engine, to_host, want_noisy):
    """signals: one list of 1-D clips per argument of the host function.  -> the host function's tuple per item (+ noisy)"""
    host_fn, names = _MIX_FORMS[form]
    signals = [list(s) for s in signals]
    n = len(signals[0])
    if any(len(s) != n for s in signals):
        raise ValueError("%s_list: lists of %s clips" % (host_fn.__name__, ", ".join(str(len(s)) for s in signals)))
    for i in range(n):
        item = [s[i] for s in signals]
        if any(len(list(c.shape)) != 1 for c in item):
            raise ValueError("%s_list: item %d: clips must be 1-d time arrays, (samples,), got %s"
                             % (host_fn.__name__, i, ", ".join(str(tuple(c.shape)) for c in item)))
        if any(c.shape[0] != item[0].shape[0] for c in item):
            raise ValueError("%s_list: item %d: the signals of one item must have one length, got %s"
                             % (host_fn.__name__, i, ", ".join(str(c.shape[0]) for c in item)))
    rng = rng if rng is not None else np.random.default_rng()
    speech = "aug" if form == 2 else "front"
    eng = engine      # the default Engine is created only when something needs the device
    out = [None] * n
    draws = {}
    for i in range(n):      # in list order: the device items' draws, the host items' calls (which draw for themselves)
        item = [s[i] for s in signals]
        if all(_clips.is_f32(c) for c in item) and item[0].shape[0] > 0:
            snr = _uniform(snr_l, snr_h, rng) if snr_l is not None and snr_h is not None else None
            draws[i] = (snr, _uniform(scale_lower, scale_upper, rng))
            continue
        res = host_fn(*[_clips.as_numpy(c) for c in item], snr_l=snr_l, snr_h=snr_h, scale_lower=scale_lower, scale_upper=scale_upper,
                      rng=rng)
        ys = list(res[:len(names)])
        if want_noisy:
            ys.append(ys[names.index("noise")] + ys[names.index(speech)])
        if not to_host:
            eng = _engine_or_default(eng)
            ys = [_clips.to_device(y, eng.device) for y in ys]
        out[i] = tuple(ys[:len(names)]) + tuple(res[len(names):]) + tuple(ys[len(names):])
    lengths = [c.shape[0] for c in signals[0]]
    for idx in _clips.batches(draws, lengths, MAX_BATCH):
        eng = _engine_or_default(eng)
        lens = [lengths[i] for i in idx]
        ld = (lens[-1] + 3) // 4 * 4      # rows 16-byte aligned: the kernels' wide loads and stores
        batch = {name: _clips.pad([s[i] for i in idx], eng.device, torch.float32, width=ld) for name, s in zip(names, signals)}
        snrs = [draws[i][0] for i in idx]
        y = eng.mix_noise(batch["front"], batch["noise"], hq=batch.get("hq"), aug=batch.get("aug"), lengths=lens,
                          noise_weight=None if snrs[0] is None else [10 ** (float(v) / 20) for v in snrs],
                          scale=[draws[i][1] for i in idx], want_noisy=want_noisy)
        cols = [_clips.unpad(y[name], lens, to_host) for name in names + (("noisy",) if want_noisy else ())]
        for j, i in enumerate(idx):
            rows = tuple(col[j] for col in cols)
            out[i] = rows[:len(names)] + draws[i] + rows[len(names):]
    return out


def add_noise_and_scale_list(front, noise, snr_l=-5, snr_h=35, scale_lower=0.6, scale_upper=1.0, rng=None, engine=None, to_host=True,
                             want_noisy=False):
    """`add_noise_and_scale` for lists of 1-D clips (item i = front[i], noise[i], of one length): `snr` then `scale` are drawn per
    item, in list order, from the one `rng` -- a seeded call consumes the generator as a loop over the single-clip function does.
    Items whose clips are all float32 (NumPy or device tensors) are sorted by length and go through Engine.mix_noise as padded
    batches of up to MAX_BATCH, bit for bit the host function; every other dtype takes the host function.
    -> one tuple per item, (front, noise, snr, scale[, noisy]); snr is None when snr_l or snr_h is; the signals are NumPy arrays
    (to_host), or device tensors that `restore_list` takes as they are.  noisy = front + noise, the model's input."""
    return _mix_list(0, (front, noise), snr_l, snr_h, scale_lower, scale_upper, rng, engine, to_host, want_noisy)


def add_noise_and_scale_with_HQ_list(HQ, front, noise, snr_l=-5, snr_h=35, scale_lower=0.6, scale_upper=1.0, rng=None, engine=None,
                                     to_host=True, want_noisy=False):
    """`add_noise_and_scale_with_HQ` for lists, as `add_noise_and_scale_list` -> (HQ, front, noise, snr, scale[, noisy]) per item.
    The device's level rule sums in float64 where NumPy sums float32 pairwise: float32 items agree with the host function to
    rounding (16 * 2^-24 relative, tests/test_gpu_mix_noise.py), not bit for bit."""
    return _mix_list(1, (HQ, front, noise), snr_l, snr_h, scale_lower, scale_upper, rng, engine, to_host, want_noisy)


def add_noise_and_scale_with_HQ_with_Aug_list(HQ, front, augfront, noise, snr_l=-5, snr_h=35, scale_lower=0.6, scale_upper=1.0, rng=None,
                                              engine=None, to_host=True, want_noisy=False):
    """`add_noise_and_scale_with_HQ_with_Aug` for lists -> (HQ, front, augfront, noise, snr, scale[, noisy]) per item, noisy =
    augfront + noise; otherwise as `add_noise_and_scale_with_HQ_list`."""
    return _mix_list(2, (HQ, front, augfront, noise), snr_l, snr_h, scale_lower, scale_upper, rng, engine, to_host, want_noisy)


def hard_clip_list(clips, threshold, engine=None, to_host=True):
    """`hard_clip` for a list of clips: float32 clips (NumPy or device tensors) through torch.clamp where they are, bit for bit
    np.clip; every other dtype takes the host function.  -> NumPy arrays (to_host), or tensors on the engine's device."""
    out = []
    for c in clips:
        y = torch.clamp(_clips.as_tensor(c), -threshold, threshold) if _clips.is_f32(c) else hard_clip(_clips.as_numpy(c), threshold)
        out.append(_clips.as_numpy(y) if to_host else _clips.to_device(y, _engine_or_default(engine).device))
    return out


# ------------------------------------------------------------------------------------------------------------------
# the array effects of MagicalEffects.effect: dataloaders/augmentation/magical_effects.py:66-108, 169-190, tools/others/audio_op.py:152-174
# and their draws, dataloaders/augmentation/random_server.py:135-217 with tools/pytorch/random_.py:36-45
# ------------------------------------------------------------------------------------------------------------------
EFFECT_TYPES = {      # RandomServer.effects_type: 0 = applied to the array, 1 / 1.1 = a sox effect of the chain, 3 = "anytime"
    "tempo": 1, "speed": 1, "fade": 1.1, "pitch": 1, "treble": 1, "bass": 1, "tremolo": 1, "clip": 1, "reverse": 1,
    "reverb_freeverb": 1, "reverb_rir": 0, "low_pass": 1, "high_pass": 1, "time_dropout": 0, "empty_c": 0, "empty_n": 0, "beep": 0,
    "quant": 0, "anytime": 3,
}
MAX_QUANT_BINS = 16      # what the device quantiser takes (Engine.MAX_QUANT_BINS)


def quantification(samples, params):
    """MagicalEffects.quantification, params = [decision, bins]: the clip divided by its peak, every sample moved DOWN to the next of
    the 2 ** bins levels linspace(-1 + 1 / level, 1 - 1 / level, level) strictly below it, times the peak -> float64.  A sample at or
    below the lowest level gets index -1, which NumPy reads as the TOP level: the negative peak -p comes out as +(1 - 1 / level) p.
    Kept.  A silent clip is 0 / 0 = NaN throughout (an invalid-value warning), NaN sorts above every level, and the top level times
    a peak of 0 is 0."""
    bins = params[1]
    level = 2 ** bins
    peak = np.max(np.abs(samples))
    samples = samples / np.max(np.abs(samples))
    space = np.linspace(start=-(1 / level) * level + (1 / level), stop=(1 / level) * level - (1 / level), num=level, endpoint=True)
    index = np.digitize(samples, space, right=True) - 1
    return space[index] * peak


def smooth(signal, smooth_center, smooth_samples=50, interval=4):
    """audio_op.smooth: the 2 * smooth_samples samples around smooth_center are replaced, all but the last `interval`, by the cubic
    interpolation through every interval-th of them -- IN PLACE; a centre closer than smooth_samples to either end leaves the signal
    as it is.  A 2-D signal is smoothed in its column 0 and returned as (samples, 1)."""
    from scipy.interpolate import interp1d
    if smooth_center < smooth_samples or signal.shape[0] - smooth_center < smooth_samples:
        return signal
    two_d = len(list(signal.shape)) > 1
    if two_d:
        signal = signal[:, 0]
    first = smooth_center - smooth_samples
    samples = signal[first:smooth_center + smooth_samples]
    xnew = np.arange(samples.shape[0])
    x = xnew[0::interval]
    xnew = xnew[:x[-1]]
    smoothed = interp1d(x, samples[0::interval], kind="cubic")(xnew)
    signal[first:first + smoothed.shape[0]] = smoothed
    return signal[:, None] if two_d else signal


_smooth_matrix = None


def smooth_matrix():
    """`smooth` with its defaults as a matrix: the 96 samples it writes are M @ knots, knots = signal[c - 50 : c + 50 : 4] as
    float64 -- cubic interpolation is linear in its knots, so column i of M (96, 25) is the interpolation of the i-th unit vector.
    Built once with SciPy; read-only.  What Engine.time_dropout hands to the library."""
    global _smooth_matrix
    if _smooth_matrix is None:
        from scipy.interpolate import interp1d
        x, xnew = np.arange(0, 100, 4), np.arange(96)
        m = np.stack([interp1d(x, e, kind="cubic")(xnew) for e in np.eye(25)], axis=1)
        m = np.ascontiguousarray(m, dtype=np.float64)
        m.setflags(write=False)
        _smooth_matrix = m
    return _smooth_matrix


def _dropout_range(length, params):
    """time_dropout's sample range: (int(length * start), int(length * start + length * trunk_length))"""
    start, trunk_length = params[1]
    return int(length * start), int(length * start + length * trunk_length)


def time_dropout(frames, params):
    """MagicalEffects.time_dropout, params = [decision, [start, trunk_length]] as fractions of the clip: that stretch is zeroed and
    both its edges are smoothed (`smooth` around the first zeroed sample, then around the first sample behind the stretch) -- IN
    PLACE, as the reference works."""
    start, end = _dropout_range(frames.shape[0], params)
    frames[start:end] = np.zeros_like(frames[start:end])
    frames = smooth(frames, smooth_center=start)
    frames = smooth(frames, smooth_center=end)
    return frames


def _array_steps(effects):
    """The type-0 effects of one item's dict in dict order, as (name, params) -- "empty_c" alone when it is among them; ValueError
    for a sox effect and for an unknown name."""
    steps = []
    for key in effects.keys():
        if key not in EFFECT_TYPES:
            raise ValueError("Unknown effect %s" % (key,))
        if EFFECT_TYPES[key] != 0:
            raise ValueError("array_effects: %s is an effect of the sox chain, which is not built here" % (key,))
        if key in ("reverb_rir", "time_dropout", "quant", "empty_c"):
            steps.append((key, effects[key]))
    return [s for s in steps if s[0] == "empty_c"][:1] or steps


def _rir_of(rirs, params):
    if rirs is None:
        raise ValueError("array_effects: reverb_rir needs the list of RIRs")
    return rirs[params[1]]


def array_effects(frames, effects, rirs=None):
    """The tail of MagicalEffects.effect (magical_effects.py:81-108) for one clip, behind the sox chain: `effects` is the dict
    name -> [decision, params] that RandomServer.generate (or `draw_array_effects`) returns, rirs the list of RIR arrays that
    effects["reverb_rir"][1] indexes.  The input is not modified; the array keeps its dtype (the reference has made it float32 by
    then).  LARGESCALE: a clip whose largest sample exceeds 10 is divided by 2 ** 15 first and multiplied by it at the end.
    "empty_c" returns zeros straight away, before that rescale.  Otherwise the type-0 effects in dict order: reverb_rir,
    time_dropout, quant; "empty_n" and "beep" are ignored, as the reference ignores them.  ValueError for a sox effect (types 1,
    1.1, 3: the chain is not built here) and for an unknown name."""
    steps = _array_steps(effects)
    frames = np.array(frames)
    large = bool(np.max(frames) > 10)
    if large:
        frames = frames / 2 ** 15
    if frames.ndim > 1:
        frames = np.squeeze(frames)
    frames, emptied = _array_tail(frames, steps, rirs)
    if large and not emptied:
        frames = frames * 2 ** 15
    return frames


def _array_tail(frames, steps, rirs):
    """`_array_steps`' steps on an array this function may modify -> (result, whether "empty_c" returned zeros)"""
    for key, params in steps:
        if key == "empty_c":
            return np.zeros_like(frames), True
        if key == "reverb_rir":
            frames = reverb_rir(frames, _clips.as_numpy(_rir_of(rirs, params)))
        elif key == "time_dropout":
            frames = time_dropout(frames, params)
        else:
            frames = quantification(frames, params)
    return frames, False


def _random_select(probs, rng):
    """random_.random_select: ONE chance for all the entries of `probs`"""
    chance = int(rng.random() * 2 ** 31)
    return [chance < p * 2 ** 31 for p in probs], chance


def draw_array_effects(n, p_effects, effect_list, rir_nums, rng):
    """RandomServer.generate(effect_list) for type-0 names, per item, in `effect_list` order, from the one generator: a name draws
    its chance (`random_select` over p_effects[name]["prob"]) and is skipped when the first decision is false; otherwise its
    parameters through `_uniform` -- reverb_rir [True, int(U(0, rir_nums))]; time_dropout [True, [start, trunk]] with start =
    U(drop_range[0], drop_range[1] - max_segment), then trunk = U(0, max_segment); quant [decisions, int(U(*bins))]; empty_c,
    empty_n, beep [True, None].  -> n dicts that `array_effects` takes."""
    out = []
    for _ in range(n):
        item = {}
        for name in effect_list:
            if EFFECT_TYPES.get(name) != 0:
                raise ValueError("draw_array_effects: %s is no array effect" % (name,))
            p = p_effects[name]
            decision, _chance = _random_select(p["prob"], rng)
            if not decision[0]:
                continue
            if name == "reverb_rir":
                item[name] = [True, int(_uniform(0, rir_nums, rng))]
            elif name == "time_dropout":
                start = _uniform(p["drop_range"][0], p["drop_range"][1] - p["max_segment"], rng)
                trunk_length = _uniform(0.0, p["max_segment"], rng)
                item[name] = [True, [start, trunk_length]]
            elif name == "quant":
                item[name] = [decision, int(_uniform(p["bins"][0], p["bins"][1], rng))]
            else:
                item[name] = [True, None]
        out.append(item)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the sox chain of MagicalEffects.effect (magical_effects.py:41-64, 110-156), as far as it is fully specified: the biquads low_pass,
# high_pass, bass and treble, clip and reverse.  RESTATED from published definitions (the RBJ audio-EQ-cookbook biquads that sox's
# biquads.c implements; WavAugment's clip) and NOT pinned: neither sox nor the `augment` package was at hand.  What is checked is what
# SciPy and torch can check (tests/test_effect_chain_host.py); a machine that has sox is what would pin it.  NOT modelled: sox's
# rounding of every sample to a multiple of 2^-31, and the six effects left out -- tempo, speed, pitch, fade, tremolo, reverb_freeverb.
# ------------------------------------------------------------------------------------------------------------------
CHAIN_BIQUADS = ("low_pass", "high_pass", "bass", "treble")
CHAIN_NOT_BUILT = ("tempo", "speed", "pitch", "fade", "tremolo", "reverb_freeverb")
SOX_MIN, SOX_MAX = -1.0, 1.0 - 2.0 ** -31      # sox's 32-bit sample range


def biquad_design(name, value, fs=44100):
    """(b0, b1, b2, a1, a2), a0 = 1, in float64 with Python's math: low_pass / high_pass -- value = the cut-off in Hz, a two-pole
    Butterworth, equal to scipy.signal.butter(2, value, fs=fs) --; bass / treble -- value = the gain in dB, a shelf of slope 0.5 around
    100 Hz / 3000 Hz: `value` dB at DC / at Nyquist, 0 dB at the other end; a gain of 0 is the identity (1, 0, 0, 0, 0).  ValueError
    unless 0 < f < fs / 2."""
    import math
    if name not in CHAIN_BIQUADS:
        raise ValueError("biquad_design: %s is no biquad of the chain" % (name,))
    f = float(value) if name in ("low_pass", "high_pass") else (100.0 if name == "bass" else 3000.0)
    if not 0 < f < fs / 2:
        raise ValueError("biquad_design: %s: the frequency %r must lie inside (0, %r)" % (name, f, fs / 2))
    w0 = 2 * math.pi * f / fs
    c, s = math.cos(w0), math.sin(w0)
    if name in ("low_pass", "high_pass"):
        alpha = s / (2 * math.sqrt(0.5))
        if name == "low_pass":
            b = ((1 - c) / 2, 1 - c, (1 - c) / 2)
        else:
            b = ((1 + c) / 2, -(1 + c), (1 + c) / 2)
        a = (1 + alpha, -2 * c, 1 - alpha)
    else:
        gain = float(value)
        if gain == 0:
            return (1.0, 0.0, 0.0, 0.0, 0.0)
        A = math.exp(gain / 40 * math.log(10))
        alpha = s / 2 * math.sqrt((A + 1 / A) * (1 / 0.5 - 1) + 2)
        q = 2 * math.sqrt(A) * alpha
        if name == "bass":
            b = (A * ((A + 1) - (A - 1) * c + q), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - q))
            a = ((A + 1) + (A - 1) * c + q, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - q)
        else:
            b = (A * ((A + 1) + (A - 1) * c + q), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - q))
            a = ((A + 1) - (A - 1) * c + q, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - q)
    return (b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0])


def _chain_steps(effects, sample_rate=44100):
    """The chain part of one item's dict as the program Engine.effect_chain takes, in `generate_effect_chain`'s order -- fade first
    (not built: ValueError), then the type-1 names in dict order: ("biquad", design), ("clip", 1 / params[1]), ("reverse",).  The
    type-0 names are the tail's.  ValueError for the six effects that are not built, for "anytime" and for an unknown name."""
    for key in effects.keys():
        if key not in EFFECT_TYPES:
            raise ValueError("Unknown effect %s" % (key,))
        if key in CHAIN_NOT_BUILT or EFFECT_TYPES[key] == 3:
            raise ValueError("chain_effects: %s is not built here" % (key,))
    steps = []
    for key in effects.keys():
        if EFFECT_TYPES[key] != 1:
            continue
        if key in CHAIN_BIQUADS:
            steps.append(("biquad", biquad_design(key, float(effects[key][1]), sample_rate)))
        elif key == "clip":
            steps.append(("clip", float(1 / effects[key][1])))
        else:
            steps.append(("reverse",))
    return steps


def _run_program(x, steps):
    """A program of `_chain_steps` on a float32 array -> float32 array (a new one)"""
    from scipy.signal import sosfilt
    k = 0
    while k < len(steps):
        if steps[k][0] == "clip":      # WavAugment's Python effect: x.clamp_(min=x.min() * factor, max=x.max() * factor) in float32
            factor = np.float32(steps[k][1])
            lo, hi = np.float32(x.min()) * factor, np.float32(x.max()) * factor
            x = np.minimum(np.maximum(x, lo), hi)
            k += 1
            continue
        w = np.clip(x.astype(np.float64), SOX_MIN, SOX_MAX)      # a sox run: up to the next clip step
        while k < len(steps) and steps[k][0] != "clip":
            if steps[k][0] == "reverse":
                w = w[::-1]
            else:
                b0, b1, b2, a1, a2 = steps[k][1]
                w = np.clip(sosfilt(np.array([[b0, b1, b2, 1.0, a1, a2]]), np.ascontiguousarray(w)), SOX_MIN, SOX_MAX)
            k += 1
        x = w.astype(np.float32)
    return np.ascontiguousarray(x)


def chain_effects(frames, effects, sample_rate=44100):
    """The sox chain of MagicalEffects.effect for one clip, as far as it is built here: `effects` is the dict name -> [decision,
    params] of RandomServer.generate (or `draw_effects`); its type-0 names are left to `array_effects`.  The clip is made float32
    (and squeezed), the input is not modified, the result is float32.  A sox run is a maximal stretch of low_pass, high_pass, bass,
    treble and reverse: the clip is widened to float64 and limited to sox's range [-1, 1 - 2^-31], every biquad is
    scipy.signal.sosfilt of `biquad_design`'s section from a zero state with its output limited again (the state keeps the unlimited
    value), reverse flips, and the run's result is rounded once to float32.  clip, between runs, clamps the float32 clip to
    [min * factor, max * factor], factor = float32(1 / params[1]), float32 products.  ValueError for tempo, speed, pitch, fade,
    tremolo, reverb_freeverb, "anytime" and unknown names.  Restated, not pinned against sox; its rounding to multiples of 2^-31 is
    not modelled."""
    steps = _chain_steps(effects, sample_rate)
    x = np.array(_clips.as_numpy(frames), dtype=np.float32)
    if x.ndim > 1:
        x = np.squeeze(x)
    return _run_program(x, steps)


def _tail_effects(effects):
    return {key: effects[key] for key in effects.keys() if EFFECT_TYPES.get(key) == 0}


def magical_effects(frames, effects, rirs=None, sample_rate=44100):
    """The whole of MagicalEffects.effect (magical_effects.py:66-108) for one clip and one drawn dict: the clip is made float32;
    LARGESCALE is decided once, on that input -- a largest sample above 10 divides the clip by 2 ** 15 here and multiplies the
    result by it at the very end --; `chain_effects`; then the type-0 tail as `array_effects` runs it ("empty_c" gives zeros).  Both
    parts are checked before anything runs."""
    steps = _chain_steps(effects, sample_rate)
    tail = _array_steps(_tail_effects(effects))
    x = np.array(_clips.as_numpy(frames), dtype=np.float32)
    large = bool(x.size and np.max(x) > 10)
    if large:
        x /= np.float32(2 ** 15)
    if x.ndim > 1:
        x = np.squeeze(x)
    x, emptied = _array_tail(_run_program(x, steps), tail, rirs)
    if large and not emptied:
        x = x * 2 ** 15
    return x


def draw_effects(n, p_effects, effect_list, rir_nums, rng):
    """RandomServer.generate(effect_list) / `do` (random_server.py:135-217) per item, for every name it knows, in `effect_list` order
    from the one generator -- consumed exactly as a loop over `do` consumes it, also for the names nothing here runs.  A name draws
    its chance and is skipped when the first decision is false; then tempo, speed, pitch [decisions, U(up range) if the second
    decision holds else U(down range)]; treble, bass, tremolo [decisions, U(level)]; clip [decisions, U(louder_time)]; low_pass,
    high_pass [decisions, U(their range)]; reverse [True, None]; fade [True, [U(in portion), U(out portion)]]; reverb_freeverb
    [True, [U(reverb_level), U(dumping_factor), U(room_size)]]; "anytime" [True, its four values]; the type-0 names as
    `draw_array_effects` draws them.  -> n dicts that `magical_effects` takes."""
    ranges = {"treble": "level", "bass": "level", "tremolo": "level", "clip": "louder_time", "low_pass": "low_pass_range",
              "high_pass": "high_pass_range"}
    out = []
    for _ in range(n):
        item = {}
        for name in effect_list:
            if name not in EFFECT_TYPES:
                raise ValueError("Unknown effect %s" % (name,))
            if EFFECT_TYPES[name] == 0:
                item.update(draw_array_effects(1, p_effects, [name], rir_nums, rng)[0])
                continue
            p = p_effects[name]
            sample = lambda key: float(_uniform(p[key][0], p[key][1], rng))      # noqa: E731
            decision, _chance = _random_select(p["prob"], rng)
            if not decision[0]:
                continue
            if name in ("tempo", "speed"):
                item[name] = [decision, sample("speed_up_range" if decision[1] else "speed_down_range")]
            elif name == "pitch":
                item[name] = [decision, sample("pitch_up_range" if decision[1] else "pitch_down_range")]
            elif name in ranges:
                item[name] = [decision, sample(ranges[name])]
            elif name == "reverse":
                item[name] = [True, None]
            elif name == "fade":
                item[name] = [True, [sample("fade_in_portion"), sample("fade_out_portion")]]
            elif name == "reverb_freeverb":
                item[name] = [True, [sample("reverb_level"), sample("dumping_factor"), sample("room_size")]]
            else:      # "anytime"
                item[name] = [True, [sample("inner_segment_scale"), sample("overall_scale"), sample("first_segment_portion"),
                                     sample("snr_range")]]
        out.append(item)
    return out


# ------------------------------------------------------------------------------------------------------------------
# batch forms of the array effects (Engine.quantize, Engine.time_dropout, csrc/effects.hip) and of the whole tail
# ------------------------------------------------------------------------------------------------------------------
_FX_DTYPES = (torch.float32, torch.float64)


def _fx_dtype(c):
    """The torch dtype of a clip the device effects take -- non-empty, 1-D, float32 or float64 -- or None"""
    if len(list(c.shape)) != 1 or c.shape[0] == 0:
        return None
    for dtype in _FX_DTYPES:
        if str(c.dtype).endswith(str(dtype).split(".")[-1]):
            return dtype
    return None


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _fx_list(clips, takes, call, host, engine, to_host):
    """What the two list forms share: the clips i with takes(i) as padded batches of one dtype (rows padded to a multiple of 4: the
    kernels' 16-byte accesses) through call(eng, x, idx, lens) -> (B, ld) tensor; every other item through host(i)."""
    lengths = [c.shape[0] if len(list(c.shape)) else 0 for c in clips]
    out = [None] * len(clips)
    eng = engine      # the default Engine is created only when something needs the device
    for dtype in _FX_DTYPES:
        dev = [i for i in range(len(clips)) if _fx_dtype(clips[i]) == dtype and takes(i)]
        for idx in _clips.batches(dev, lengths, MAX_BATCH):
            eng = _engine_or_default(eng)
            lens = [lengths[i] for i in idx]
            x = _clips.pad([clips[i] for i in idx], eng.device, dtype, width=(lens[-1] + 3) // 4 * 4)
            for i, row in zip(idx, _clips.unpad(call(eng, x, idx, lens), lens, to_host)):
                out[i] = row
    for i in range(len(clips)):
        if out[i] is None:
            y = host(i)
            if not to_host:
                eng = _engine_or_default(eng)
                y = _clips.to_device(y, eng.device)
            out[i] = y
    return out


def quantification_list(clips, bins, engine=None, to_host=True):
    """`quantification` for a list of clips, bins one int for all or one per clip.  Non-empty 1-D float32 and float64 clips (NumPy or
    device tensors) whose bins is an int in 0..16 are grouped by dtype, sorted by length and go through Engine.quantize as padded
    batches of up to MAX_BATCH, bit for bit the host function; every other item takes the host function.  -> list in the caller's
    order: float64 NumPy arrays (to_host), or device tensors."""
    clips = list(clips)
    bins = _per_clip(bins, len(clips), "quantification_list: bins")
    return _fx_list(clips, lambda i: _is_int(bins[i]) and 0 <= bins[i] <= MAX_QUANT_BINS,
                    lambda eng, x, idx, lens: eng.quantize(x, [int(bins[i]) for i in idx], lengths=lens)[0],
                    lambda i: quantification(_clips.as_numpy(clips[i]), [True, bins[i]]), engine, to_host)


def time_dropout_list(clips, params, engine=None, to_host=True):
    """`time_dropout` for a list of clips, params = [decision, [start, trunk_length]] for all or one such per clip.  The sample range
    of every clip is computed on the host exactly as the single-clip function computes it; non-empty 1-D float32 and float64 clips
    with 0 <= start <= end go through Engine.time_dropout as padded batches of up to MAX_BATCH -- bit for bit the host function
    outside the two smoothed patches, inside them to the rounding of a 25-term float64 sum (tests/test_gpu_array_effects.py) --,
    every other item takes the host function on a copy.  The inputs are never modified.  -> list in the caller's order, each in
    its clip's dtype: NumPy arrays (to_host), or device tensors."""
    clips = list(clips)
    params = list(params)
    if not (params and isinstance(params[0], (list, tuple))):      # one [decision, [start, trunk_length]] for all
        params = [params] * len(clips)
    if len(params) != len(clips):
        raise ValueError("time_dropout_list: params: %d entries for %d clips" % (len(params), len(clips)))
    ranges = [_dropout_range(c.shape[0], p) if len(list(c.shape)) else (0, -1) for c, p in zip(clips, params)]
    return _fx_list(clips, lambda i: 0 <= ranges[i][0] <= ranges[i][1],
                    lambda eng, x, idx, lens: eng.time_dropout(x, [ranges[i][0] for i in idx], [ranges[i][1] for i in idx], lengths=lens),
                    lambda i: time_dropout(np.array(_clips.as_numpy(clips[i])), params[i]), engine, to_host)


def array_effects_list(clips, effects, rirs=None, engine=None, to_host=True):
    """`array_effects` for a list of clips, effects[i] the dict of clip i.  Non-empty 1-D float32 and float64 clips stay on the
    device from their first effect to the end: the LARGESCALE division and multiplication by 2 ** 15 and "empty_c" are exact torch
    operations where the clip is; then, step position by step position, the clips whose next type-0 effect is the same are handed
    together to `reverb_rir_list`, `time_dropout_list` or `quantification_list` with to_host=False -- exactly the composition of
    those three --, and the results come down in one download per dtype at the end.  Every other clip takes `array_effects`.  All
    the dicts are checked before anything runs.  -> list in the caller's order: NumPy arrays (to_host), or device tensors."""
    clips = list(clips)
    effects = list(effects)
    if len(effects) != len(clips):
        raise ValueError("array_effects_list: %d dicts for %d clips" % (len(effects), len(clips)))
    steps = [_array_steps(e) for e in effects]
    eng = engine
    cur = [None] * len(clips)
    large = [False] * len(clips)
    chain = []      # the clips that walk the device chain
    for i, c in enumerate(clips):
        if _fx_dtype(c) is None:
            cur[i] = array_effects(_clips.as_numpy(c), effects[i], rirs)
            continue
        t = _clips.as_tensor(c)
        large[i] = bool(torch.max(t) > 10)
        if steps[i] and steps[i][0][0] == "empty_c":
            cur[i] = torch.zeros_like(t)
            large[i] = False      # (returned before the rescale; zeros either way)
            continue
        cur[i] = t / 2 ** 15 if large[i] else t
        chain.append(i)
    for pos in range(max([len(steps[i]) for i in chain], default=0)):
        for name in ("reverb_rir", "time_dropout", "quant"):
            idx = [i for i in chain if len(steps[i]) > pos and steps[i][pos][0] == name]
            if not idx:
                continue
            eng = _engine_or_default(eng)
            group, par = [cur[i] for i in idx], [steps[i][pos][1] for i in idx]
            if name == "reverb_rir":
                if rirs is None:
                    raise ValueError("array_effects: reverb_rir needs the list of RIRs")
                ys = reverb_rir_list(group, rirs, rir_index=[p[1] for p in par], engine=eng, to_host=False)
            elif name == "time_dropout":
                ys = time_dropout_list(group, par, engine=eng, to_host=False)
            else:
                ys = quantification_list(group, [p[1] for p in par], engine=eng, to_host=False)
            for i, y in zip(idx, ys):
                cur[i] = y
    for i in chain:
        if large[i]:
            cur[i] = cur[i] * 2 ** 15
    if not to_host:
        for i in range(len(clips)):
            eng = _engine_or_default(eng)
            cur[i] = _clips.to_device(cur[i], eng.device)
        return cur
    for dtype in _FX_DTYPES:      # one download per dtype for what is on the device
        idx = [i for i in range(len(clips)) if isinstance(cur[i], torch.Tensor) and cur[i].is_cuda and cur[i].dtype == dtype]
        if idx:
            lens = [cur[i].shape[0] for i in idx]
            for i, row in zip(idx, _clips.unpad(_clips.pad([cur[i] for i in idx], cur[idx[0]].device, dtype), lens, True)):
                cur[i] = row
    return [_clips.as_numpy(c) for c in cur]


# ------------------------------------------------------------------------------------------------------------------
# batch forms of the chain (Engine.effect_chain, csrc/chain.hip) and of the whole of MagicalEffects.effect
# ------------------------------------------------------------------------------------------------------------------
def _chain_on_device(clips, programs, eng, large=None):
    """clips[i] (1-D, non-empty; any dtype: made float32 where it is) through programs[i] on the device -> float32 device rows, each
    bit for bit `_run_program`.  large[i]: the clip is divided by 2 ** 15 first (LARGESCALE; exact torch division).  Padded batches
    of up to MAX_BATCH sorted by length; a row with a sample that is not finite is computed by the host function instead."""
    lengths = [c.shape[0] for c in clips]
    out = [None] * len(clips)
    for idx in _clips.batches(range(len(clips)), lengths, MAX_BATCH):
        lens = [lengths[i] for i in idx]
        rows = [_clips.as_tensor(clips[i]).to(device=eng.device, dtype=torch.float32) for i in idx]
        if large is not None:
            rows = [r / 2 ** 15 if large[i] else r for i, r in zip(idx, rows)]
        x = _clips.pad(rows, eng.device, torch.float32, width=(lens[-1] + 3) // 4 * 4)
        finite = torch.isfinite(x).all(dim=1).tolist()      # (one download per batch)
        y = eng.effect_chain(x, [programs[i] for i in idx], lengths=lens)
        for j, (i, row) in enumerate(zip(idx, _clips.unpad(y, lens, False))):
            out[i] = row if finite[j] else _clips.to_device(_run_program(rows[j].cpu().numpy(), programs[i]), eng.device)
    return out


def _chain_takes(c, program):
    """Whether the device chain takes this clip and its program: non-empty and 1-D, a program inside Engine.effect_chain's limits"""
    from .engine import Engine
    return len(list(c.shape)) == 1 and c.shape[0] > 0 and Engine.effect_chain_supported(program)


def chain_effects_list(clips, effects, engine=None, to_host=True):
    """`chain_effects` for a list of clips, effects[i] the dict of clip i.  Non-empty 1-D clips -- float32 after the reference's
    conversion, which `chain_effects` applies to every dtype -- whose program the device takes (at most 8 steps; a dict cannot hold
    more) go through Engine.effect_chain as padded batches of up to MAX_BATCH, sorted by length, every clip with its own program:
    bit for bit `chain_effects`.  Every other clip, and a clip with a sample that is not finite, takes the host function.  All the
    dicts are checked before anything runs.  -> list in the caller's order: float32 NumPy arrays (to_host), or device tensors."""
    clips = list(clips)
    effects = list(effects)
    if len(effects) != len(clips):
        raise ValueError("chain_effects_list: %d dicts for %d clips" % (len(effects), len(clips)))
    programs = [_chain_steps(e) for e in effects]
    eng = _engine_or_default(engine)
    dev = [i for i in range(len(clips)) if _chain_takes(clips[i], programs[i])]
    out = [None] * len(clips)
    for i, row in zip(dev, _chain_on_device([clips[i] for i in dev], [programs[i] for i in dev], eng)):
        out[i] = row
    for i in range(len(clips)):
        if out[i] is None:
            out[i] = chain_effects(clips[i], effects[i])
    return _deliver(out, eng, to_host)


def _deliver(rows, eng, to_host):
    """Results that are device tensors or host arrays -> all on the device, or all NumPy arrays after one download per dtype"""
    if not to_host:
        return [_clips.to_device(r, eng.device) for r in rows]
    rows = list(rows)
    for dtype in _FX_DTYPES:
        idx = [i for i, r in enumerate(rows) if isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == dtype and r.dim() == 1
               and r.shape[0] > 0]
        if idx:
            lens = [rows[i].shape[0] for i in idx]
            for i, row in zip(idx, _clips.unpad(_clips.pad([rows[i] for i in idx], rows[idx[0]].device, dtype), lens, True)):
                rows[i] = row
    return [_clips.as_numpy(r) for r in rows]


def magical_effects_list(clips, effects, rirs=None, engine=None, to_host=True):
    """`magical_effects` for a list of clips, effects[i] the dict of clip i: device-resident from the first step to the last.  A
    non-empty 1-D clip whose program the device takes is made float32 where it is, LARGESCALE is decided there and its division is an
    exact torch operation, the chain runs through Engine.effect_chain (`chain_effects_list`'s batches), and the float32 rows go on,
    without leaving the device, through `array_effects_list`'s steps for the type-0 names; the multiplication by 2 ** 15 comes last.
    Bit for bit `magical_effects` wherever `array_effects_list` is bit for bit `array_effects`: through LARGESCALE, "empty_c" and the
    quantiser; the device reverb rounds its sums otherwise than SciPy (inside its own bound, `reverb_rir_list`), and time_dropout's
    smoothed patches agree to rounding.  Every other clip takes `magical_effects`.  All the dicts are checked before anything runs.
    -> list in the caller's order: NumPy arrays (to_host), or device tensors."""
    clips = list(clips)
    effects = list(effects)
    if len(effects) != len(clips):
        raise ValueError("magical_effects_list: %d dicts for %d clips" % (len(effects), len(clips)))
    programs = [_chain_steps(e) for e in effects]
    tails = [_tail_effects(e) for e in effects]
    for t in tails:
        _array_steps(t)
    eng = _engine_or_default(engine)
    dev = [i for i in range(len(clips)) if _chain_takes(clips[i], programs[i])]
    out = [None] * len(clips)
    if dev:
        rows = [_clips.as_tensor(clips[i]).to(device=eng.device, dtype=torch.float32) for i in dev]
        large = [bool(v) for v in (_clips.pad(rows, eng.device, torch.float32).max(dim=1).values > 10).tolist()]
        # (a padded row's zeros cannot lift a maximum above 10)
        chained = _chain_on_device(rows, [programs[i] for i in dev], eng, large=large)
        # `array_effects_list` decides LARGESCALE for itself on what it is given.  The chain never raises a clip's largest sample
        # above max(it, 1), so only a clip that was above 10 * 2 ** 15 can still be above 10 here: such a row takes the host tail
        emptied = [[s[0] for s in _array_steps(tails[i])][:1] == ["empty_c"] for i in dev]
        over = [bool(v) for v in (_clips.pad(chained, eng.device, torch.float32).max(dim=1).values > 10).tolist()]
        keep = [j for j in range(len(dev)) if not over[j]]
        done = dict(zip(keep, array_effects_list([chained[j] for j in keep], [tails[dev[j]] for j in keep], rirs, engine=eng,
                                                 to_host=False)))
        for j, i in enumerate(dev):
            if over[j]:      # (rare: the host tail, which takes the steps without the LARGESCALE decision)
                y = _clips.to_device(_array_tail(chained[j].cpu().numpy(), _array_steps(tails[i]), rirs)[0], eng.device)
            else:
                y = done[j]
            out[i] = y * 2 ** 15 if large[j] and not emptied[j] else y
    for i in range(len(clips)):
        if out[i] is None:
            out[i] = magical_effects(clips[i], effects[i], rirs)
    return _deliver(out, eng, to_host)
