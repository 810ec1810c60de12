"""Host-side mirror of the reference's model objects for the inference hot path.

Same names, argument meaning and error behaviour as the reference surface that
``handler()`` uses, backed by libvfx.so instead of torch.nn:

    model = VoiceFixer(hp, channels=2, type_target="vocals").load_from_checkpoint(ckpt)
    model.eval(); model = model.to(device)
    sp, cos, sin = model.f_helper.wav_to_spectrogram_phase(wav)      # fDomainHelper.py:67-89
    mel = model.mel(sp.permute(0,1,3,2)).permute(0,1,3,2)            # mel_scale.py:52-64
    out = model(mel)['mel']                                          # gsr_voicefixer.py:183-193
    wav = model.vocoder(from_log(out))                               # eval_gsr_voicefixer.py:66

and for the waveform-out ResUNets (models/ssr_unet.py:145-155, models/gsr_unet.py):

    out = model(sp, wav)   ->  {'wav': (B,1,L), 'clean': sp}

Tensors are torch tensors on the ROCm device; the batch dimension may be > 1 (the
reference only ever passes 1).  There is no CPU path: constructing a model on a
non-GPU device raises.
"""
import math
import pickle

import numpy as np
import torch

from . import clips
from .engine import Engine, MODEL_DNN_MEL, MODEL_GRU_MEL, MODEL_UNET_MEL, MODEL_UNET_SPEC, MODEL_VOCODER

EPS = 1e-8


# ----------------------------------------------------------------------------------------
# tools/pytorch/pytorch_util.py:157-163 (elementwise glue, kept in torch on the device)
# ----------------------------------------------------------------------------------------
def to_log(input):
    assert torch.sum(input < 0) == 0, str(input) + " has negative values counts " + str(torch.sum(input < 0))
    return torch.log10(torch.clip(input, min=1e-8))


def from_log(input):
    return 10 ** torch.clip(input, max=5)


def tensor2numpy(tensor):
    return tensor.detach().cpu().numpy()


def _hp_get(hp, *keys, default=None):
    cur = hp
    for k in keys:
        try:
            cur = cur[k]
        except Exception:
            cur = getattr(cur, k, None)
        if cur is None:
            return default
    return cur


class MelScale:
    """tools/pytorch/mel_scale.py:10-64 -- HTK triangular filterbank applied to (..., freq, time)."""

    def __init__(self, engine, n_mels=128, sample_rate=44100, f_min=0.0, f_max=None, n_stft=1025, norm=None,
                 mel_scale="htk"):
        if n_mels != 128 or n_stft != 1025 or norm is not None or mel_scale != "htk" or f_min != 0.0:
            raise ValueError("libvfx implements the reference configuration only (128 HTK bands over 1025 bins)")
        self.engine = engine
        self.n_mels, self.sample_rate = n_mels, sample_rate
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.fb = self.filterbank(n_stft, n_mels, sample_rate, self.f_max)
        engine.set_mel_filterbank(self.fb)

    @staticmethod
    def filterbank(n_freqs, n_mels, sample_rate, f_max):
        """float32 torch-CPU evaluation of the HTK filterbank with the reference's operation
        order (mel_scale.py:131-221), so the table is bit-identical to the reference buffer."""
        hz = torch.linspace(0, sample_rate // 2, n_freqs)
        to_mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
        edges_mel = torch.linspace(to_mel(0.0), to_mel(f_max), n_mels + 2)
        edges = 700.0 * (10.0 ** (edges_mel / 2595.0) - 1.0)
        span = edges[1:] - edges[:-1]
        delta = edges.unsqueeze(0) - hz.unsqueeze(1)
        lower = (-1.0 * delta[:, :-2]) / span[:-1]
        upper = delta[:, 2:] / span[1:]
        return torch.max(torch.zeros(1), torch.min(lower, upper))

    def __call__(self, specgram):
        x = specgram.transpose(-1, -2).contiguous()           # (..., time, freq)
        return self.engine.mel_project(x).transpose(-1, -2)   # (..., n_mels, time)

    forward = __call__


class FDomainHelper:
    """tools/pytorch/modules/fDomainHelper.py:11-113 for subband=None (the only configuration any
    call site uses, fDomainHelper.py:20,25)."""

    def __init__(self, engine, window_size=2048, hop_size=441, center=True, pad_mode="reflect", window="hann",
                 freeze_parameters=True, subband=None):
        if subband is not None:
            raise NotImplementedError("PQMF sub-band analysis is outside the hot path (its filter files are not in the reference)")
        if (window_size, hop_size, pad_mode, window) != (2048, 441, "reflect", "hann") or not center:
            raise ValueError("libvfx implements the reference STFT configuration only (2048/441/hann/reflect/center)")
        self.engine = engine

    def _flat(self, input):
        B, C, L = input.shape
        return input.reshape(B * C, L), (B, C)

    def spectrogram_phase(self, input, eps=0.0):
        """(B, L) -> mag, cos, sin (B, 1, T, 1025); mag = sqrt(clamp(re^2 + im^2, eps, inf)), cos = re / mag,
        sin = im / mag (fDomainHelper.py:60-65; with the reference's default eps = 0 an exactly silent bin gives
        0 / 0 = NaN phases there, as in the reference)."""
        o = self.engine.stft(input, want_mel=False, want_sp=True, want_phase=True, eps=eps)
        return o["sp"][:, None], o["cos"][:, None], o["sin"][:, None]

    def wav_to_spectrogram_phase(self, input, eps=1e-8):
        x, (B, C) = self._flat(input)
        o = self.engine.stft(x, want_mel=False, want_sp=True, want_phase=True, eps=eps)
        shp = (B, C) + tuple(o["sp"].shape[1:])
        return o["sp"].reshape(shp), o["cos"].reshape(shp), o["sin"].reshape(shp)

    def wav_to_spectrogram(self, input, eps=1e-8):
        x, (B, C) = self._flat(input)
        sp = self.engine.stft(x, want_mel=False, want_sp=True, eps=eps)["sp"]
        return sp.reshape((B, C) + tuple(sp.shape[1:]))

    def wav_to_mel(self, input, log10=False):
        """Fused front-end (no (B,C,T,1025) round trip through HBM): (B,C,L) -> (B,C,T,128)."""
        x, (B, C) = self._flat(input)
        mel = self.engine.stft(x, want_mel=True, log10_mel=log10)["mel"]
        return mel.reshape((B, C) + tuple(mel.shape[1:]))

    def istft(self, real, imag, length):
        """(B,1,T,1025) x2 -> (B, length)   [torchlibrosa ISTFT via fDomainHelper.py:30-32]."""
        return self.engine.istft(real[:, 0], imag[:, 0], length)

    def spectrogram_phase_to_wav(self, sps, coss, sins, length):
        B, C = sps.shape[:2]
        flat = lambda t: t.reshape((B * C,) + tuple(t.shape[2:]))
        return self.engine.istft(flat(sps * coss), flat(sps * sins), length).reshape(B, C, length)


class Vocoder:
    """`voicefixer.Vocoder(sample_rate=44100)`: linear mel (B,1,T,128) -> wave (B,1,(T+T%2+4)*441)."""

    def __init__(self, engine, sample_rate=44100):
        assert sample_rate == 44100
        self.engine = engine
        self.rate = sample_rate

    def load_state_dict(self, sd, prefix=""):
        self.engine.load_state_dict(MODEL_VOCODER, fold_weight_norm(sd), prefix)

    def load_from_checkpoint(self, ckpt):
        """The pip package keeps its own generator file beside the Lightning checkpoint (the reference constructs
        `Vocoder(sample_rate=44100)`, models/gsr_voicefixer.py:113, and the weights come from the package cache): a
        `{'generator': state_dict}` container (read_checkpoint), weight-norm pairs folded here, a DataParallel `module.` prefix
        dropped."""
        sd = read_checkpoint(ckpt)
        if sd and all(k.startswith("module.") for k in sd):
            sd = {k[len("module."):]: v for k, v in sd.items()}
        self.load_state_dict(sd)
        return self

    def __call__(self, mel, cuda=None, check=True):
        """`check` = False defers the flag check (one device sync) to the caller: Engine.check_flags, once per file in
        the handlers."""
        assert mel.size()[-1] == 128
        out = self.engine.vocoder(mel[:, 0])
        # only the 16-bit mode can raise a flag here (saturation); the negative-input flag belongs to the UNet stage's prep
        # kernel.  The reference's vocoder has no assert and no sync: precision 0 / 1 pay none either.
        if check and self.engine.precision == 2:
            out = _rerun_if_saturated(self.engine, out, lambda e: e.vocoder(mel[:, 0]))
        return out[:, None]

    forward = __call__


def _rerun_if_saturated(engine, out, call):
    """Every arithmetic mode: a negative value that reached a log10 raises like `to_log`'s assert.  16-bit vocoder
    (precision 2): an activation beyond the fp16 range is clamped by the kernels and reported through a sticky device flag;
    such a call is re-run on the split-bf16 twin of the engine, so the mode is never silently wrong on weights whose
    activations do not fit fp16 (Engine.check_flags: one device sync per call, like `to_log`'s assert)."""
    again = engine.check_flags(call)
    return out if again is None else again


def fold_weight_norm(sd):
    """Replace (weight_g, weight_v) pairs by the plain weight g * v / ||v|| (norm over dims != 0)."""
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_g"):
            base = k[:-len("weight_g")]
            vv = sd[base + "weight_v"].float()
            norm = vv.reshape(vv.shape[0], -1).norm(dim=1).reshape((-1,) + (1,) * (vv.dim() - 1))
            out[base + "weight"] = v.float() * vv / norm
        elif k.endswith("weight_v"):
            continue
        else:
            out[k] = v
    return out


# Lightning checkpoints (`save_hyperparameters()`, models/gsr_voicefixer.py:106) pickle `hyper_parameters` with project
# classes (tools.utils.HParams, ...) that are not importable here, so `torch.load(weights_only=True)` refuses them.
# The fallback below never imports or calls anything the file names: globals on a short allow-list (tensor rebuild
# helpers, storage types, plain containers) resolve normally, EVERY other global becomes an inert stand-in class that
# swallows its constructor arguments and state.  A hostile file can therefore not run code through this reader; what
# it can do is fail to load.
_SAFE_GLOBALS = {
    ("collections", "OrderedDict"), ("collections", "defaultdict"),
    ("builtins", "dict"), ("builtins", "list"), ("builtins", "tuple"), ("builtins", "set"), ("builtins", "frozenset"),
    ("builtins", "int"), ("builtins", "float"), ("builtins", "bool"), ("builtins", "str"), ("builtins", "bytes"),
    ("builtins", "complex"), ("builtins", "slice"), ("builtins", "range"), ("builtins", "bytearray"),
    ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_tensor"), ("torch._utils", "_rebuild_parameter"),
    ("torch._utils", "_rebuild_parameter_with_state"), ("torch._tensor", "_rebuild_from_type_v2"),
    ("torch", "Size"), ("torch", "device"), ("torch", "Tensor"), ("torch.nn.parameter", "Parameter"),
    ("torch.serialization", "_get_layout"), ("_codecs", "encode"),
    ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"), ("numpy", "dtype"),
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray"),
}


def _is_safe_global(module, name):
    if (module, name) in _SAFE_GLOBALS:
        return True
    if module == "torch" and (name.endswith("Storage") or name in (
            "float32", "float64", "float16", "bfloat16", "int64", "int32", "int16", "int8", "uint8", "bool")):
        return True
    return False


class _Inert(dict):
    """Stand-in for a class / function the checkpoint names but this reader does not trust or cannot import."""

    def __init__(self, *args, **kwargs):
        dict.__init__(self)

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.update(state)

    def __reduce_ex__(self, protocol):
        return (dict, (dict(self),))

    # list- / set-like reducers (append, extend, add) of stubbed containers
    def append(self, *a):
        pass

    def extend(self, *a):
        pass

    def add(self, *a):
        pass


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if _is_safe_global(module, name):
            return super().find_class(module, name)
        return type(str(name), (_Inert,), {"__module__": "voicefixer_main_amd.models"})


class _PickleModule:
    Unpickler = _Unpickler
    load = staticmethod(lambda f, **kw: _Unpickler(f, **kw).load())
    __name__ = "pickle"


def _load_checkpoint_obj(path):
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        return torch.load(path, map_location="cpu", weights_only=False, pickle_module=_PickleModule)


def _checkpoint_hp(obj):
    """The `hyper_parameters["hp"]` a Lightning checkpoint object saved (`save_hyperparameters()`, gsr_voicefixer.py:106), or None."""
    hyper = obj.get("hyper_parameters") if isinstance(obj, dict) else None
    return _hp_get(hyper, "hp") if hyper is not None else None


def _state_dict_of(obj, path):
    sd = obj
    for key in ("state_dict", "generator", "model"):
        if isinstance(obj, dict) and isinstance(obj.get(key), dict) and obj[key] and \
                all(isinstance(v, torch.Tensor) for v in obj[key].values()):
            sd = obj[key]
            break
    if not isinstance(sd, dict) or not sd or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError("%s holds no state_dict of tensors" % path)
    return sd


def read_checkpoint(path):
    """Lightning .ckpt (``{'state_dict': ..., 'hyper_parameters': ...}``, eval_gsr_voicefixer.py:33), a GAN-style container
    (``{'generator': state_dict, ...}``: the pip vocoder's own file; ``{'model': ...}``) or a bare state_dict file ->
    state_dict of CPU tensors.  Tries torch's `weights_only` reader first; a file that only fails there because it pickles
    project classes is re-read with the allow-listing unpickler above (nothing the file names is imported or executed)."""
    return _state_dict_of(_load_checkpoint_obj(path), path)


def _resample_list(engine, wavs, sample_rate):
    """A list of 1-D clips at `sample_rate` -> the same clips at the engine's rate (44.1 kHz), resampled on the device as ONE padded
    batch with their lengths (every clip's values are those of its own resample_poly call).  An empty list (the ranks other
    than the source of a distributed restore_list) and clips already at 44.1 kHz pass through."""
    sr_out = engine.cfg.sample_rate
    if int(sample_rate) == sr_out or not wavs:
        return wavs
    lengths = [int(w.shape[-1]) for w in wavs]
    batch = clips.pad([w.reshape(-1) for w in wavs], engine.device, torch.float32, width=max(max(lengths), 1))
    y, out_lengths = engine.resample(batch, sample_rate, sr_out, lengths=lengths)
    return clips.unpad(y, out_lengths, to_host=False)


# the keys of the dict a handler returns for a file with a target (eval_gsr_voicefixer.py:59-64, eval_ssr_unet.py:121-126), in the
# column order of Engine.restore_gsr_varlen_scored / restore_ssr_varlen_scored
HANDLER_METRIC_KEYS = ("mel-lsd", "mel-sispec", "mel-non-log-sispec", "mel-ssim")
MIN_SCORED_SAMPLES = 6 * 441   # 7 STFT frames: skimage's 7 x 7 SSIM refuses a smaller mel image


MIN_VALIDATED_SAMPLES = 1025   # more than n_fft / 2 samples: the STFT's reflect padding


def _paired_batches(engine, wavs, targets, max_batch, bucket_key, bucket_len, name, min_samples, min_why, what="scored", how="restored"):
    """The list layer under restore_scored_list and validate_list: checks a list of clips and their targets, then yields the padded
    batches to run -- clips sorted by length (longest first, as dist.restore_sharded_lengths orders restore_list's), up to
    `max_batch` of one `bucket_key` per batch, both padded to `bucket_len(longest)` -- as (chunk = the clips' indices in the input
    list, x (B, Lmax), lengths, t (B, Lmax), target_lengths)."""
    from . import dist as vdist
    if vdist.world_rank()[0] > 1:
        raise RuntimeError("%s: %s sets are %s by one process (a process group of %d ranks is initialised)"
                           % (name, what, how, vdist.world_rank()[0]))
    if len(wavs) != len(targets):
        raise ValueError("%s: %d clips and %d targets" % (name, len(wavs), len(targets)))
    hop = engine.hop
    lengths = [int(w.shape[-1]) for w in wavs]
    tlens = [int(t.shape[-1]) for t in targets]
    for i, (n, m) in enumerate(zip(lengths, tlens)):
        if n < min_samples:
            raise ValueError("%s: clip %d has %d samples: %s at least %d (%s)" % (name, i, n, min_why[0], min_samples, min_why[1]))
        if n // hop != m // hop:
            raise ValueError("%s: clip %d has %d frames but its target has %d" % (name, i, n // hop + 1, m // hop + 1))
    buckets = {}
    for i, n in enumerate(lengths):
        buckets.setdefault(bucket_key(n), []).append(i)
    for k in sorted(buckets, reverse=True):
        idx = sorted(buckets[k], key=lambda i: (-lengths[i], i))
        for a in range(0, len(idx), max_batch):
            chunk = idx[a:a + max_batch]
            lens, tl = [lengths[i] for i in chunk], [tlens[i] for i in chunk]
            width = bucket_len(max(lens))
            x = clips.pad([wavs[i].reshape(-1) for i in chunk], engine.device, torch.float32, width=width)
            t = clips.pad([targets[i].reshape(-1) for i in chunk], engine.device, torch.float32, width=width)
            yield chunk, x, lens, t, tl


def _restore_scored_list(engine, call, wavs, targets, max_batch, bucket_key, bucket_len, name):
    """The two restore_scored_list methods over _paired_batches: `call(x, lengths, t, target_lengths)` -> (restored (B, Lmax),
    scores (B, 4) on the device).  ONE device-to-host copy of the (B, 4) block per batch.  -> (restored clips, [{key: score}]) in
    input order."""
    restored, scores = [None] * len(wavs), [None] * len(wavs)
    for chunk, x, lens, t, tl in _paired_batches(engine, wavs, targets, max_batch, bucket_key, bucket_len, name, MIN_SCORED_SAMPLES,
                                                 ("the scores need", "7 STFT frames")):
        out, block = call(x, lens, t, tl)
        block = block.cpu().tolist()     # the batch's one device-to-host copy of scores
        for j, i in enumerate(chunk):
            restored[i] = out[j, :lens[j]]
            scores[i] = {key: float(v) for key, v in zip(HANDLER_METRIC_KEYS, block[j])}
    return restored, scores


def _validate_list(engine, call, wavs, targets, max_batch, bucket_key, bucket_len, name, equal_lengths=False):
    """The two validate_list methods over _paired_batches: `call(x, lengths, t, target_lengths)` -> the loss per clip, (B,) float64 on
    the device.  ONE device-to-host copy per batch.  -> ([loss per file] in input order, their mean: what Lightning logs as val_l
    for an epoch of the reference's batch_size = 1 validation loader)."""
    if equal_lengths:
        for i, (w, t) in enumerate(zip(wavs, targets)):
            if int(w.shape[-1]) != int(t.shape[-1]):
                raise ValueError("%s: clip %d has %d samples but its target has %d: the spectrogram losses compare equal lengths"
                                 % (name, i, int(w.shape[-1]), int(t.shape[-1])))
    if len(wavs) == 0 and len(targets) == 0:
        raise ValueError("%s: no clips" % name)
    losses = [None] * len(wavs)
    for chunk, x, lens, t, tl in _paired_batches(engine, wavs, targets, max_batch, bucket_key, bucket_len, name, MIN_VALIDATED_SAMPLES,
                                                 ("the STFT needs", "more than n_fft / 2: reflect padding"), "validation", "scored"):
        block = call(x, lens, t, tl).cpu().tolist()     # the batch's one device-to-host copy
        for j, i in enumerate(chunk):
            losses[i] = float(block[j])
    return losses, math.fsum(losses) / len(losses)


def _restore_prefiltered_list(model, wavs, threshold, kwargs):
    """The list layer under the two restore_prefiltered_list methods: detect each clip's bandwidth (simulate.band_cutoff_list), low-pass
    it there (simulate.lowpass_each(..., 44100, 5, "stft"): eval_ssr_unet.py:105-106), restore (the model's own restore_list).  The clips
    are device tensors from the first step on; what comes to the host is the cut-offs, one copy per detector batch.  A clip whose
    cut-off is 0 Hz -- silence -- goes in unfiltered: int(ratio * 44100) = 0 is no rate to resample to."""
    from . import simulate
    eng = model.engine
    sample_rate = kwargs.pop("sample_rate", 44100)
    wavs = _resample_list(eng, list(wavs), sample_rate)      # the detector and the filter are defined at 44.1 kHz
    wavs = [clips.as_tensor(w).reshape(-1).to(device=eng.device, dtype=torch.float32) for w in wavs]
    cutoffs = simulate.band_cutoff_list(wavs, eng.cfg.sample_rate, threshold, engine=eng)
    keep = [i for i, c in enumerate(cutoffs) if c > 0]
    if keep:
        low = simulate.lowpass_each([wavs[i] for i in keep], [cutoffs[i] for i in keep], eng.cfg.sample_rate, 5, "stft", engine=eng,
                                    to_host=False)
        for i, y in zip(keep, low):
            wavs[i] = y
    return model.restore_list(wavs, **kwargs), cutoffs


def _restore_spliced_list(model, wavs, cut_bins, threshold, ramp, match, max_gain_db, kwargs):
    """The list layer under the two restore_spliced_list methods: resample to 44.1 kHz, take each clip's cut-off bin from the bandwidth
    detector (splice.cut_bins_list) unless the caller gave them, restore the UNFILTERED clips (the model's own restore_list), splice each
    result onto its input (splice.splice_list).  The clips are device tensors from the first step on.  Under torch.distributed the
    splice runs on the rank that holds restore_list's gathered outputs; the other ranks return (None, None)."""
    from . import simulate, splice
    eng = model.engine
    sample_rate = kwargs.pop("sample_rate", 44100)
    wavs = _resample_list(eng, list(wavs), sample_rate)      # the detector and the splice are defined at 44.1 kHz
    wavs = [clips.as_tensor(w).reshape(-1).to(device=eng.device, dtype=torch.float32) for w in wavs]
    if cut_bins is None:
        bins = splice.cut_bins_list(wavs, threshold, engine=eng)
    else:
        bins = [int(cut_bins)] * len(wavs) if np.ndim(cut_bins) == 0 else [int(c) for c in cut_bins]
        if len(bins) != len(wavs):
            raise ValueError("restore_spliced_list: %d cut-off bins for %d clips" % (len(bins), len(wavs)))
    restored = model.restore_list(wavs, **kwargs)
    if restored is None:
        return None, None
    outs, gains = splice.splice_list(wavs, restored, bins, ramp=ramp, match=match, max_gain_db=max_gain_db, engine=eng)
    info = [{"cut_bin": c, "cutoff_hz": simulate.band_cutoff_hz(c, eng.cfg.sample_rate), "gain": g} for c, g in zip(bins, gains)]
    return outs, info


MIN_RESTORE_SAMPLES = 1025     # more than n_fft / 2 samples: the shortest clip restore_list takes (the STFT's reflect padding)


def trimmed_span(bounds, n, least=MIN_RESTORE_SAMPLES):
    """The span of a clip of n samples that restore_trimmed_list restores, from what trim_empty keeps of it, (start, stop): a span of
    fewer than `least` samples is widened to `least`, first to the right, then to the left, within the clip; a clip that is itself
    shorter goes in whole."""
    start, stop = bounds
    if n < least:
        return 0, n
    if stop - start < least:
        stop = min(n, start + least)
        start = max(0, stop - least)
    return start, stop


def _restore_trimmed_list(model, wavs, threshold, frame_length, kwargs):
    """The list layer under the two restore_trimmed_list methods: find what trim_empty keeps of every clip on the device
    (activity.trim_empty_bounds_list: the bounds come to the host, one copy per batch; the samples stay), restore those spans in ONE
    restore_list call, write each into zeros of its clip's length.  A clip trim_empty returns None for never reaches the network."""
    from . import activity
    eng = model.engine
    sample_rate = kwargs.pop("sample_rate", 44100)
    wavs = _resample_list(eng, list(wavs), sample_rate)      # the segment length is defined at 44.1 kHz
    wavs = [clips.as_tensor(w).reshape(-1).to(device=eng.device, dtype=torch.float32) for w in wavs]
    found = activity.trim_empty_bounds_list(wavs, threshold, eng.cfg.sample_rate, frame_length, engine=eng)
    bounds = [None if b is None else trimmed_span(b, int(w.shape[0])) for b, w in zip(found, wavs)]
    outs = [torch.zeros_like(w) for w in wavs]
    keep = [i for i, b in enumerate(bounds) if b is not None]
    if keep:
        restored = model.restore_list([wavs[i][bounds[i][0]:bounds[i][1]] for i in keep], **kwargs)
        for i, y in zip(keep, restored or []):       # (None on the ranks of a distributed restore_list that do not hold the result)
            outs[i][bounds[i][0]:bounds[i][1]] = y
    return outs, bounds


def _wave_batch(batch, key, name):
    """batch[key] of the reference's validation loader, (B, L, 1) or (B, L) -> (B, L)."""
    x = batch[key]
    if x.dim() == 3 and x.shape[-1] == 1:
        x = x[..., 0]
    if x.dim() != 2:
        raise ValueError("%s: batch['%s'] must be (B, L, 1) or (B, L), got %s" % (name, key, tuple(batch[key].shape)))
    return x


class _Base:
    def __init__(self, hp=None, channels=1, type_target="vocals", device="cuda:0", engine=None):
        self.hp = hp
        self.channels = channels
        self.type_target = type_target
        self.engine = engine if engine is not None else Engine(device)
        self.device = self.engine.device
        self.sampling_rate = _hp_get(hp, "data", "sampling_rate", default=44100)
        self.f_helper = FDomainHelper(
            self.engine,
            window_size=_hp_get(hp, "model", "window_size", default=2048),
            hop_size=_hp_get(hp, "model", "hop_size", default=441),
            center=True,
            pad_mode=_hp_get(hp, "model", "pad_mode", default="reflect"),
            window=_hp_get(hp, "model", "window", default="hann"))
        self.mel = MelScale(self.engine, n_mels=_hp_get(hp, "model", "mel_freq_bins", default=128),
                            sample_rate=self.sampling_rate,
                            n_stft=_hp_get(hp, "model", "window_size", default=2048) // 2 + 1)
        self.vocoder = Vocoder(self.engine, sample_rate=44100)
        self.training = False

    # nn.Module-ish surface the handlers touch
    def eval(self):
        self.training = False
        return self

    def to(self, device):
        if torch.device(device).type != "cuda":
            raise RuntimeError("this model only runs on the MI355X (requested %s)" % device)
        return self

    def get_vocoder(self):
        return self.vocoder

    def get_f_helper(self):
        return self.f_helper

    def pre(self, input):
        sp, _, _ = self.f_helper.wav_to_spectrogram_phase(input)
        mel_orig = self.mel(sp.permute(0, 1, 3, 2)).permute(0, 1, 3, 2)
        return sp, mel_orig

    def load_from_checkpoint(self, ckpt):
        self.load_state_dict(read_checkpoint(ckpt))
        return self


ANALYSIS_PREFIX = "generator.analysis_module."
ANALYSIS_SWITCHES = ("unet", "unet_small", "bi_gru", "dnn")   # the order Generator.__init__ tests them (gsr_voicefixer.py:46-87)
ANALYSIS_MODEL_IDS = {"unet": MODEL_UNET_MEL, "bi_gru": MODEL_GRU_MEL, "dnn": MODEL_DNN_MEL}
_MODULE_OF_ID = {v: k for k, v in ANALYSIS_MODEL_IDS.items()}


def analysis_module_from_keys(keys, prefix=ANALYSIS_PREFIX):
    """'unet', 'bi_gru' or 'dnn' by the state-dict keys of Generator.analysis_module, or None when there are none."""
    keys = list(keys)
    has = lambda sfx: any(k == prefix + sfx or k == sfx for k in keys)
    if has("2.gru.weight_hh_l0"):
        return "bi_gru"
    if has("14.weight"):
        return "dnn"
    if any(k.startswith(prefix + "encoder_block1.") or k.startswith("encoder_block1.") for k in keys):
        return "unet"
    return None


def analysis_module_from_hp(hp):
    """The module Generator.__init__ builds for `hp` ('unet_small' is the same network as 'unet'), or None when `hp` has no
    switches or switches none on (Generator.__init__ then builds no module: nothing to cross-check).  Refuses mel_freq_bins != 128."""
    sw = _hp_get(hp, "task", "gsr", "gsr_model", "voicefixer")
    if sw is None:
        return None
    n_mel = _hp_get(hp, "model", "mel_freq_bins", default=128)
    if int(n_mel) != 128:
        raise ValueError("mel_freq_bins = %s: the analysis modules are implemented for 128 mel bins only" % n_mel)
    for name in ANALYSIS_SWITCHES:
        if _hp_get(sw, name, default=False):
            return "unet" if name == "unet_small" else name
    return None


def select_analysis_module(keys, hp=None, ckpt_hp=None, prefix=ANALYSIS_PREFIX):
    """The analysis module of a VoiceFixer checkpoint: decided by its weights, cross-checked against the model's hp and the hp the
    checkpoint saved.  A switch that disagrees with the weights raises ValueError naming both."""
    by_keys = analysis_module_from_keys(keys, prefix)
    for what, h in (("hp", hp), ("the checkpoint's hyper_parameters['hp']", ckpt_hp)):
        if h is None:
            continue
        by_hp = analysis_module_from_hp(h)
        if by_hp is not None and by_keys is not None and by_hp != by_keys:
            raise ValueError("%s selects the '%s' analysis module but the weights are those of '%s'" % (what, by_hp, by_keys))
    return by_keys


class VoiceFixer(_Base):
    """models/gsr_voicefixer.py:93-193 (inference surface): analysis module (mel ResUNet, bi_gru or dnn) + TFGAN vocoder."""

    unet_prefix = ANALYSIS_PREFIX

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._ckpt_hp = None

    @property
    def analysis_module(self):
        """'unet', 'bi_gru' or 'dnn': the module the ENGINE has selected (the one source of truth: a model built on another
        handle -- the handlers' split-bf16 twin -- runs what that handle selected)."""
        return _MODULE_OF_ID[self.engine.analysis_model]

    def load_from_checkpoint(self, ckpt):
        obj = _load_checkpoint_obj(ckpt)        # read once: the state_dict and the hp the checkpoint saved
        self._ckpt_hp = _checkpoint_hp(obj)
        try:
            self.load_state_dict(_state_dict_of(obj, ckpt))
        finally:
            self._ckpt_hp = None
        return self

    def load_state_dict(self, sd, strict=True):
        keys = list(sd.keys())
        module = select_analysis_module(keys, self.hp, self._ckpt_hp, self.unet_prefix)
        if module in ("bi_gru", "dnn"):
            mid = ANALYSIS_MODEL_IDS[module]
            if any(k.startswith(self.unet_prefix) for k in keys):
                self.engine.load_state_dict(mid, sd, self.unet_prefix)
            else:
                self.engine.load_state_dict(mid, {k: v for k, v in sd.items() if k[:1].isdigit()})
            self.engine.select_analysis(mid)
        elif any(k.startswith(self.unet_prefix) for k in keys):
            self.engine.load_state_dict(MODEL_UNET_MEL, sd, self.unet_prefix)
        elif any(k.startswith("encoder_block1.") for k in keys):
            self.engine.load_state_dict(MODEL_UNET_MEL, sd)
        elif strict:
            raise KeyError("no ResUNet weights ('%s*') in the state_dict" % self.unet_prefix)
        if module == "unet" and self.engine.analysis_model != MODEL_UNET_MEL:
            self.engine.select_analysis(MODEL_UNET_MEL)
        for pfx in ("vocoder.model.", "vocoder."):
            sub = {k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx)}
            if any(k.startswith("condnet.") for k in sub):
                self.vocoder.load_state_dict(sub)
                break
        if "mel.fb" in sd:
            self.engine.set_mel_filterbank(sd["mel.fb"])
        return self

    def forward(self, mel_orig, check=True):
        """mel_orig (B,1,T,128) linear, non-negative -> {'mel': log10 estimate}  (Generator.forward,
        gsr_voicefixer.py:86-91).  `check` reproduces to_log's assert (one device sync)."""
        mid = self.engine.analysis_model
        if mid != MODEL_UNET_MEL:
            out = self.engine.analysis_mel(mid, mel_orig[:, 0])[:, None]
        else:
            out = self.engine.resunet_mel(mel_orig[:, 0])[:, None]
        if check:
            # to_log's assert; a saturation bit left by a deferred vocoder check (Vocoder.__call__(check=False), raw engine calls)
            # is NOT consumed here -- it stays raised for that check
            self.engine.check_negative_input()
        return {"mel": out}

    __call__ = forward

    def restore(self, wav, unify_energy=False, sample_rate=44100):
        """Fused handler() segment body: wav (B,1,L) or (B,L) -> restored wav of the same shape, at 44.1 kHz.  Input at another
        `sample_rate` is resampled on the device first (Engine.resample: resample_poly's values, as librosa.load(path, 44100))."""
        squeeze = wav.dim() == 3
        x = wav[:, 0] if squeeze else wav
        if int(sample_rate) != self.engine.cfg.sample_rate:
            x, _ = self.engine.resample(x, sample_rate, self.engine.cfg.sample_rate)
        out = self.engine.restore_gsr(x, unify_energy=unify_energy)
        out = _rerun_if_saturated(self.engine, out, lambda e: e.restore_gsr(x, unify_energy=unify_energy))
        return out[:, None] if squeeze else out

    def restore_list(self, wavs, unify_energy=False, max_batch=128, sample_rate=44100):
        """A test set of clips of ARBITRARY lengths (what the reference's harness iterates, one handler call per file:
        evaluation_proc/eval.py:119-134): list of 1-D tensors -> list of restored 1-D tensors in the same order.  The clips go
        through the library sorted by length, up to `max_batch` per call, as padded batches with their lengths
        (vfx_restore_gsr_varlen: every clip's result is the one its own batch-of-one call gives; inside a call the mel ResUNet
        runs once per padded frame count over all its clips, the vocoder per run of clips of similar length); with
        torch.distributed initialised the list is dealt over the ranks by length and gathered on rank 0
        (dist.restore_sharded_lengths).  The 16-bit mode's re-run guarantee holds per batch.  Clips at another `sample_rate` are
        resampled to 44.1 kHz on the device first, as one batch with their lengths (_resample_list); the results are at 44.1 kHz."""
        from . import dist as vdist
        wavs = _resample_list(self.engine, wavs, sample_rate)
        fn = vdist.checked_restore(self.engine, unify_energy=unify_energy)
        return vdist.restore_sharded_lengths(fn, wavs, self.device, max_batch=max_batch)

    def restore_prefiltered_list(self, wavs, threshold=0.95, **kwargs):
        """restore_list behind the reference's "remove the empty upper band first" step (eval_ssr_unet.py:105-106, tools/utils.py:33-44):
        every clip's cut-off = the frequency below which `threshold` of its log-spectral energy lies, detected on the device
        (Engine.band_energy), the clip low-passed there by lowpass(clip, cutoff, 44100, 5, "stft"), then restore_list, which takes
        `kwargs` (a `sample_rate` other than 44.1 kHz is resampled first).  -> (restored clips, [cut-off in Hz per clip]) in input order.
        A silent clip (cut-off 0) is restored unfiltered."""
        return _restore_prefiltered_list(self, wavs, threshold, kwargs)

    def restore_spliced_list(self, wavs, cut_bins=None, threshold=0.95, ramp=8, match=64, max_gain_db=12.0, **kwargs):
        """restore_list for BANDWIDTH EXTENSION of clean, band-limited input (8 / 16 kHz material, low-passed recordings): the band
        below a clip's cut-off was fine to begin with, so the result keeps the input there and takes the restored clip above it.
        Every clip's cut-off bin is the bandwidth detector's (Engine.band_energy at `threshold`) unless `cut_bins` gives them; the
        unfiltered clips go through restore_list, which takes `kwargs` (a `sample_rate` other than 44.1 kHz is resampled first); then
        splice.splice_list: a cross-fade of `ramp` STFT bins under the cut-off, the restored clip level-matched to the input over the
        `match` bins under the ramp, within +-`max_gain_db` (match=0: no level match).  -> (outs, info) in input order, info[i] =
        {"cut_bin", "cutoff_hz", "gain"}.  NOT for full-band noisy input: there the detector's cut-off lies near Nyquist and the splice
        hands back mostly the input, noise included."""
        return _restore_spliced_list(self, wavs, cut_bins, threshold, ramp, match, max_gain_db, kwargs)

    def restore_trimmed_list(self, wavs, threshold=500 / 2 ** 15, frame_length=0.02, **kwargs):
        """restore_list of the ACTIVE span of every clip: leading and trailing silence, as the reference's trim_empty finds it
        (tools/others/audio_op.py:107-109: window peaks below `threshold` in segments of `frame_length` seconds; 500 / 2**15 is its
        default of 500 on the float scale), costs no network time.  The bounds are found on the device (Engine.trim_bounds), a span
        shorter than restore_list's minimum is widened (trimmed_span), the spans go through ONE restore_list call, which takes
        `kwargs`.  -> (outs, bounds) in input order: outs[i] has the length of clip i (at 44.1 kHz), zeros outside
        bounds[i] = (start, stop), the restored span inside -- bit for bit restore_list of that span; bounds[i] is None and outs[i]
        all zeros for a clip trim_empty returns None for (silence, or activity only in the segments its rules drop)."""
        return _restore_trimmed_list(self, wavs, threshold, frame_length, kwargs)

    def restore_scored_list(self, wavs, targets, unify_energy=False, max_batch=128):
        """restore_list for a test set WITH targets (every reference test list is `source target` pairs): lists of 1-D clips at
        44.1 kHz -> (restored clips, [{"mel-lsd", "mel-sispec", "mel-non-log-sispec", "mel-ssim"} per clip]) in input order -- the
        clips restore_list gives, and for each the dict handler() returns for that file (eval_gsr_voicefixer.py:56-64), scored on
        the device inside the batched call (Engine.restore_gsr_varlen_scored) instead of one segment per call with four
        device-to-host copies each.  A target must have its clip's frame count (len // 441) and a clip at least 2646 samples.
        Single process: raises when a process group of more than one rank is initialised."""
        eng = self.engine
        if not eng.supports_varlen():
            raise RuntimeError("restore_scored_list: this engine cannot run padded batches (Engine.supports_varlen)")
        call = lambda x, lens, t, tl: eng.restore_gsr_varlen_scored_checked(x, lens, t, tl, unify_energy=unify_energy)
        return _restore_scored_list(eng, call, wavs, targets, max_batch, lambda L: 0, lambda L: eng.padded_frames(L) * eng.hop - 1,
                                    "VoiceFixer.restore_scored_list")

    def validation_step(self, batch, batch_idx=0):
        """models/gsr_voicefixer.py:264-277, forward value only: batch["noisy"], batch["vocals"] (B, L, 1) or (B, L) ->
        {"loss": val_l}, the 0-dim float64 tensor L1(model(mel(noisy))['mel'], to_log(mel(vocals))) -- the number the training
        script logs as val_l and writes into the checkpoint's file name.  The library computes it per clip, without the vocoder
        (Engine.validate_gsr_varlen); the batch's value is the mean of the clips', which for the equal lengths of a batch is the
        reference's batch mean."""
        x, t = _wave_batch(batch, "noisy", "VoiceFixer.validation_step"), _wave_batch(batch, "vocals", "VoiceFixer.validation_step")
        if x.shape != t.shape:
            raise ValueError("VoiceFixer.validation_step: noisy %s and vocals %s differ in shape" % (tuple(x.shape), tuple(t.shape)))
        return {"loss": self.engine.validate_gsr_varlen(x, [int(x.shape[1])] * int(x.shape[0]), t).mean()}

    def validate_list(self, wavs, targets, max_batch=128):
        """val_l of a validation set of (noisy, vocals) pairs of ARBITRARY lengths: lists of 1-D clips at 44.1 kHz -> ([val_l per
        file] in input order, their mean).  The mean is what Lightning logs for an epoch of the reference's validation loader
        (batch_size = 1).  The files go through the library as restore_scored_list's do (sorted by length, up to `max_batch` per
        call, padded with their lengths), one device-to-host copy per batch, and never reach the vocoder.  A target must have its
        clip's frame count (len // 441) and a clip more than 1024 samples.  Single process."""
        eng = self.engine
        call = lambda x, lens, t, tl: eng.validate_gsr_varlen(x, lens, t, tl)
        return _validate_list(eng, call, wavs, targets, max_batch, lambda L: 0, lambda L: eng.padded_frames(L) * eng.hop - 1,
                              "VoiceFixer.validate_list")


class SSR_UNet(_Base):
    """models/ssr_unet.py:56-155 / models/gsr_unet.py (identical inference surface): the
    spectrogram-domain ResUNet of models/components/unet_v2.py."""

    unet_prefix = "generator.unet."

    def load_state_dict(self, sd, strict=True):
        keys = list(sd.keys())
        if any(k.startswith(self.unet_prefix) for k in keys):
            sub = {k: v for k, v in sd.items() if ".f_helper." not in k}
            self.engine.load_state_dict(MODEL_UNET_SPEC, sub, self.unet_prefix)
        elif any(k.startswith("encoder_block1.") for k in keys):
            self.engine.load_state_dict(MODEL_UNET_SPEC, {k: v for k, v in sd.items() if not k.startswith("f_helper.")})
        elif strict:
            raise KeyError("no ResUNet weights ('%s*') in the state_dict" % self.unet_prefix)
        return self

    def forward(self, sp, wav):
        """sp (B,1,T,1025) magnitude, wav (B,1,L) -> {'wav': (B,1,L), 'clean': sp}."""
        out = self.engine.resunet_spec(sp[:, 0], wav[:, 0])
        return {"wav": out[:, None], "clean": sp}

    __call__ = forward

    def restore_list(self, wavs, max_batch=16, sample_rate=44100):
        """A test set of clips of ARBITRARY lengths through `pre` + `forward` (eval_ssr_unet.py:77-114, one handler call per file
        in the reference): list of 1-D tensors -> list of restored 1-D tensors in the same order.  Clips whose frame counts pad
        to the same multiple of 64 share one call of the library as a padded batch with their lengths (vfx_restore_ssr_varlen);
        with torch.distributed initialised the list is dealt over the ranks (dist.restore_sharded_lengths).  Clips at another
        `sample_rate` are resampled to 44.1 kHz on the device first (_resample_list); the results are at 44.1 kHz."""
        from . import dist as vdist
        eng = self.engine
        wavs = _resample_list(eng, wavs, sample_rate)

        def fn(x, lengths=None):
            if lengths is None:
                return eng.resunet_spec(eng.stft(x, want_mel=False, want_sp=True)["sp"], x)
            return eng.restore_ssr_varlen(x, lengths)
        fn.bucket_key = eng.padded_frames
        fn.bucket_len = lambda L: eng.padded_frames(L) * eng.hop - 1      # one plan per (B, bucket), cf. dist.checked_restore
        return vdist.restore_sharded_lengths(fn, wavs, self.device, max_batch=max_batch)

    def restore_prefiltered_list(self, wavs, threshold=0.95, **kwargs):
        """restore_list with each clip low-passed at its own detected bandwidth first, the two lines eval_ssr_unet.py:105-106 keeps in
        front of the model: -> (restored clips, [cut-off in Hz per clip]) in input order (cf. VoiceFixer.restore_prefiltered_list)."""
        return _restore_prefiltered_list(self, wavs, threshold, kwargs)

    def restore_spliced_list(self, wavs, cut_bins=None, threshold=0.95, ramp=8, match=64, max_gain_db=12.0, **kwargs):
        """restore_list for bandwidth extension of clean, band-limited input: the input below each clip's detected cut-off, the
        super-resolved clip above it, cross-faded and level-matched: -> (outs, info) in input order (cf.
        VoiceFixer.restore_spliced_list; not for full-band noisy input, which the splice would mostly hand back)."""
        return _restore_spliced_list(self, wavs, cut_bins, threshold, ramp, match, max_gain_db, kwargs)

    def restore_trimmed_list(self, wavs, threshold=500 / 2 ** 15, frame_length=0.02, **kwargs):
        """restore_list of the active span of every clip, zeros around it: -> (outs, bounds) in input order (cf.
        VoiceFixer.restore_trimmed_list)."""
        return _restore_trimmed_list(self, wavs, threshold, frame_length, kwargs)

    def restore_scored_list(self, wavs, targets, max_batch=16):
        """restore_list for a test set with targets: -> (restored clips, [{"mel-lsd", "mel-sispec", "mel-non-log-sispec", "mel-ssim"}
        per clip]) in input order, the dict handler_ssr_unet's reference returns per file (eval_ssr_unet.py:116-126), scored inside
        the batched call (Engine.restore_ssr_varlen_scored).  Clips at 44.1 kHz; single process (cf. VoiceFixer.restore_scored_list)."""
        eng = self.engine
        return _restore_scored_list(eng, eng.restore_ssr_varlen_scored, wavs, targets, max_batch, eng.padded_frames,
                                    lambda L: eng.padded_frames(L) * eng.hop - 1, "SSR_UNet.restore_scored_list")

    VALIDATE_AGAINST = ("target", "input")

    def _l1_sp_call(self, against, name):
        """(x, lengths, t, target_lengths) -> l1_sp per clip (B,) float64 on the device, of the restored clips against `against`;
        restored and compared on the device, no host copy in between."""
        if against not in self.VALIDATE_AGAINST:
            raise ValueError("%s: against must be one of %s, got %r" % (name, self.VALIDATE_AGAINST, against))
        eng = self.engine
        return lambda x, lens, t, tl: eng.spec_losses(eng.restore_ssr_varlen(x, lens), t if against == "target" else x, lens)[:, 1]

    def validation_step(self, batch, batch_idx=0, against="target"):
        """validation_step of models/ssr_unet.py:227-234 and models/gsr_unet.py:225-232, forward value only: batch["noisy"],
        batch["vocals"] (B, L, 1) or (B, L) -> {"loss": the 0-dim float64 tensor get_loss_function("l1_sp")(estimate, reference)},
        the mean of the clips' own values (for the equal lengths of a batch: the reference's batch mean).
          against="target" (default)  l1_sp(estimate, vocals): the training objective (ssr_unet.py:220, gsr_unet.py:218)
          against="input"             l1_sp(estimate, noisy): what gsr_unet.py:230 logs as val_l -- it compares with the degraded input
        ssr_unet.py:232 hands L1_Sp the target's SPECTROGRAM (sp_target) where it expects a waveform; that line is not reproduced."""
        name = "SSR_UNet.validation_step"
        x, t = _wave_batch(batch, "noisy", name), _wave_batch(batch, "vocals", name)
        if x.shape != t.shape:
            raise ValueError("%s: noisy %s and vocals %s differ in shape" % (name, tuple(x.shape), tuple(t.shape)))
        x, t = x.to(self.device, torch.float32).contiguous(), t.to(self.device, torch.float32).contiguous()
        lens = [int(x.shape[1])] * int(x.shape[0])
        return {"loss": self._l1_sp_call(against, name)(x, lens, t, lens).mean()}

    def validate_list(self, wavs, targets, max_batch=16, against="target"):
        """validation_step over a validation set of (noisy, vocals) pairs of ARBITRARY lengths: lists of 1-D clips at 44.1 kHz ->
        ([l1_sp per file] in input order, their mean: what Lightning logs for an epoch at the reference's batch_size = 1).
        `against` as in validation_step.  A clip and its target must have EQUAL length (L1_Sp compares equal shapes) of more than
        1024 samples.  The files are bucketed as restore_list's, restored by Engine.restore_ssr_varlen and compared by
        Engine.spec_losses on the device; one device-to-host copy per batch.  Single process."""
        eng = self.engine
        return _validate_list(eng, self._l1_sp_call(against, "SSR_UNet.validate_list"), wavs, targets, max_batch, eng.padded_frames,
                              lambda L: eng.padded_frames(L) * eng.hop - 1, "SSR_UNet.validate_list", equal_lengths=True)


GSR_UNet = SSR_UNet
