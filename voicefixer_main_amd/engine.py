"""Thin Python wrapper over one libvfx handle: torch tensors in, torch tensors out.

All compute happens in the HIP library; this file only allocates outputs with torch,
passes raw device pointers + the current HIP stream, and raises on any failure.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import MODEL_DNN_MEL, MODEL_FRONTEND, MODEL_GRU_MEL, MODEL_UNET_MEL, MODEL_UNET_SPEC, MODEL_VOCODER  # noqa: F401

ANALYSIS_MODELS = (MODEL_UNET_MEL, MODEL_GRU_MEL, MODEL_DNN_MEL)

N_BINS = 1025
N_MELS = 128


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev_f32(t, device):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _host(a):
    """A host float32 C-contiguous array (None stays None): what the op_* entry points take their weights as."""
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _hptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _clip_rows(x, lengths, name=None, what="lengths"):
    """The argument handling every clip-batch method shares: x (B, L) or (L,) and each row's length (default L)
    -> (x as (B, L), whether x was 1-D, B, L, lengths as a list of ints).  With `name`, a list of another size than B raises."""
    squeeze = x.dim() == 1
    if squeeze:
        x = x[None]
    B, L = x.shape
    lengths = [L] * B if lengths is None else [int(v) for v in lengths]
    if name is not None and len(lengths) != B:
        raise ValueError("%s: %d %s for %d clips" % (name, len(lengths), what, B))
    return x, squeeze, B, L, lengths


def _float_rows(x, device, name, other):
    """x (B, L) or (L,), a tensor or anything NumPy takes -> a contiguous float32 or float64 tensor on `device`.  `other` is what
    any other dtype does: a dtype -- x is converted to it --, or an exception class -- it is raised."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    if x.dtype not in (torch.float32, torch.float64):
        if not isinstance(other, torch.dtype):
            raise other("%s: x must be float32 or float64, got %s" % (name, x.dtype))
        x = x.to(other)
    if x.dim() not in (1, 2):
        raise ValueError("%s: x must be (B, L) or (L,), got %s" % (name, tuple(x.shape)))
    return x.to(device).contiguous()


def _per_clip(v, B, cast, name=None, what=None):
    """One value for every clip, or one per clip -> a list of cast(value).  With `name`, a list of another size than B raises."""
    v = [cast(v)] * B if np.ndim(v) == 0 else [cast(u) for u in v]
    if name is not None and len(v) != B:
        raise ValueError("%s: %d %s for %d clips" % (name, len(v), what, B))
    return v


def _result_rows(_y, shape, dtype, device, name):
    """The result tensor of a method whose kernels write every element of it (zeros at and past a clip's length): a new one, or the
    caller's `_y` when it is what a new one would be."""
    if _y is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if _y.shape != shape or _y.dtype != dtype or not _y.is_contiguous() or _y.device != device:
        raise ValueError("%s: _y must be a contiguous %s %s tensor on %s" % (name, tuple(shape), dtype, device))
    return _y


class Engine:
    """One libvfx handle on one GPU (not thread-safe, like the reference's module-level model)."""

    def __init__(self, device="cuda:0", config=None):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("voicefixer_main_amd runs on an MI355X GPU only (got device %s); "
                               "there is no CPU path" % device)
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible to PyTorch")
        torch.cuda.init()
        self.cfg = _lib.VfxConfig()
        self.lib.vfx_default_config(ctypes.byref(self.cfg))
        if config:
            for k, v in config.items():
                cur = getattr(self.cfg, k)
                if hasattr(cur, "__len__"):
                    for i, x in enumerate(v):
                        cur[i] = x
                else:
                    setattr(self.cfg, k, v)
        h = ctypes.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.vfx_create(idx, ctypes.byref(self.cfg), ctypes.byref(h)), "vfx_create")
        self.h = h
        self.loaded = set()
        self._state = {}        # model id -> (state_dict, prefix) as loaded, for the stricter-arithmetic twin
        self._strict = None
        self.analysis_model = MODEL_UNET_MEL   # what restore_gsr(_varlen) runs (select_analysis)
        self._resample_taps = {}   # (up, down) -> the filter of resample_poly on the device
        self._stoi_taps = {}       # (up, down) -> Octave's resample filter (float64) on the device, for `stoi`
        self._score16k_fb = False  # the 16 kHz scoring filterbank has been handed to the library (_score_tables)
        self._resample_each_cache = collections.OrderedDict()   # (M, dtype) -> resample_poly's unscaled filter on the device, LRU

    def close(self):
        if getattr(self, "_strict", None) is not None:
            self._strict.close()
            self._strict = None
        if getattr(self, "h", None):
            self.lib.vfx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def hop(self):
        return self.cfg.hop

    def frames(self, L):
        return L // self.cfg.hop + 1

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, model, state_dict, prefix=""):
        """Upload a (reference-keyed) state_dict for `model` and finalize it."""
        n = 0
        for k, v in state_dict.items():
            if prefix:
                if not k.startswith(prefix):
                    continue
                k = k[len(prefix):]
            if k.endswith("num_batches_tracked"):
                continue
            a = np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v),
                                     dtype=np.float32)
            shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            _lib.check(self.lib.vfx_load_tensor(self.h, model, k.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim),
                       "vfx_load_tensor(%s)" % k)
            n += 1
        if n == 0:
            raise RuntimeError("no tensors with prefix %r in the state_dict" % prefix)
        _lib.check(self.lib.vfx_finalize_weights(self.h, model), "vfx_finalize_weights")
        self.loaded.add(model)
        self._state[model] = (state_dict, prefix)
        if self._strict is not None:
            self._strict.load_state_dict(model, state_dict, prefix)

    @property
    def precision(self):
        return int(self.cfg.precision)

    def strict_twin(self):
        """A second handle on the same device with the same weights in split-bf16 arithmetic (precision 1): what a call
        is re-run on when the 16-bit vocoder reports a clamped activation (VFX_FLAG_F16_SATURATED)."""
        if self._strict is None:
            cfg = {f[0]: getattr(self.cfg, f[0]) for f in self.cfg._fields_}
            cfg = {k: (list(v) if hasattr(v, "__len__") else v) for k, v in cfg.items()}
            cfg["precision"] = 1
            twin = Engine(self.device, config=cfg)
            for model, (sd, prefix) in self._state.items():
                twin.load_state_dict(model, sd, prefix)
            if self.analysis_model != MODEL_UNET_MEL:
                twin.select_analysis(self.analysis_model)
            self._strict = twin
        return self._strict

    def set_mel_filterbank(self, fb):
        self.load_state_dict(MODEL_FRONTEND, {"mel.fb": fb})

    def reserve(self, model, B, T):
        _lib.check(self.lib.vfx_reserve(self.h, model, B, T), "vfx_reserve")

    def unpin_plans(self):
        """Every hipGraph captured from this handle has been destroyed: its plans may be evicted and the arena may grow again
        (a handle with a captured plan refuses to move its arena: reserve() the largest shape before capturing)."""
        _lib.check(self.lib.vfx_unpin_plans(self.h), "vfx_unpin_plans")

    def replay(self, graph):
        """Replay a torch.cuda.CUDAGraph captured from this engine's calls on the current stream, inside the device's turn:
        captured calls are exempt from the library's one-stream-at-a-time rule (vfx.h, "Turns"), their replay is not a call of
        the library -- this brackets it so that it cannot overlap a live call on another stream of the device."""
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        s = self._stream()
        _lib.check(self.lib.vfx_turn_begin(idx, s), "vfx_turn_begin")
        try:
            graph.replay()
        finally:
            _lib.check(self.lib.vfx_turn_end(idx, s), "vfx_turn_end")

    def workspace_bytes(self, model, B, T):
        return int(self.lib.vfx_workspace_bytes(self.h, model, B, T))

    def take_flags(self, mask=None):
        """Read and clear the sticky device flags (one device sync); with `mask`, only those bits -- the others stay raised."""
        f = ctypes.c_int(0)
        if mask is None:
            _lib.check(self.lib.vfx_take_flags(self.h, self._stream(), ctypes.byref(f)), "vfx_take_flags")
        else:
            _lib.check(self.lib.vfx_take_flags_masked(self.h, self._stream(), int(mask), ctypes.byref(f)), "vfx_take_flags_masked")
        return f.value

    # ------------------------------------------------------------------ stages
    def stft(self, wav, want_mel=True, want_sp=False, want_phase=False, log10_mel=False, eps=1e-8):
        """wav (B, L) -> dict with any of mel (B,T,128), sp / cos / sin (B,T,1025).  `eps` is the clamp on the power
        (fDomainHelper.py:60-65); the fused mel output exists for the handlers' eps = 1e-8 only."""
        wav = _dev_f32(wav, self.device)
        B, L = wav.shape
        T = self.frames(L)
        eps = float(eps)
        if eps < 0.0:
            raise ValueError("eps must be >= 0")
        out = {}
        if want_mel:
            if eps != 1e-8:
                raise ValueError("the fused mel output is defined for eps = 1e-8 (wav_to_spectrogram_phase) only")
            out["mel"] = torch.empty((B, T, N_MELS), device=self.device, dtype=torch.float32)
        if want_sp:
            out["sp"] = torch.empty((B, T, N_BINS), device=self.device, dtype=torch.float32)
        if want_phase:
            out["cos"] = torch.empty((B, T, N_BINS), device=self.device, dtype=torch.float32)
            out["sin"] = torch.empty((B, T, N_BINS), device=self.device, dtype=torch.float32)
        if eps == 1e-8:
            _lib.check(self.lib.vfx_stft_mel(self.h, _ptr(wav), B, L, _ptr(out.get("mel")), _ptr(out.get("sp")),
                                             _ptr(out.get("cos")), _ptr(out.get("sin")), int(log10_mel), self._stream()),
                       "vfx_stft_mel")
        else:
            _lib.check(self.lib.vfx_stft_phase(self.h, _ptr(wav), B, L, _ptr(out.get("sp")), _ptr(out.get("cos")),
                                               _ptr(out.get("sin")), eps, self._stream()), "vfx_stft_phase")
        return out

    def mel_project(self, sp):
        """sp (..., 1025) -> (..., 128)."""
        sp = _dev_f32(sp, self.device)
        rows = sp.numel() // N_BINS
        mel = torch.empty(sp.shape[:-1] + (N_MELS,), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_mel_project(self.h, _ptr(sp), rows, _ptr(mel), self._stream()), "vfx_mel_project")
        return mel

    def istft(self, re, im, length):
        re, im = _dev_f32(re, self.device), _dev_f32(im, self.device)
        B, T, _ = re.shape
        wav = torch.empty((B, length), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_istft(self.h, _ptr(re), _ptr(im), B, T, length, _ptr(wav), self._stream()), "vfx_istft")
        return wav

    def stft_lowpass(self, x, cut_bins, lengths=None):
        """The "stft_hard" low-pass of a padded batch in ONE launch (vfx_stft_lowpass): x (B, L) or (L,), clip b = the first
        lengths[b] samples of row b (default L; 1024 < lengths[b] <= L); cut_bins: the first bin set to zero, one int or one per clip
        (>= 0; 1025 and above masks nothing).  -> float32 of the same shape on the device, rows zero past their length.  Row b is bit
        for bit simulate.stft_hard_lowpass_v0 of its first lengths[b] samples with int(1025 * ratio) == cut_bins[b], whatever batch
        it is in."""
        x = _dev_f32(x, self.device)
        if x.dim() not in (1, 2):
            raise ValueError("stft_lowpass: x must be (B, L) or (L,), got %s" % (tuple(x.shape),))
        x, squeeze, B, L, lengths = _clip_rows(x, lengths, "stft_lowpass")
        cut_bins = _per_clip(cut_bins, B, int, "stft_lowpass", "cut-off bins")
        if B == 0:
            raise ValueError("stft_lowpass: %d cut-off bins for %d clips" % (len(cut_bins), B))
        y = torch.empty((B, L), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_stft_lowpass(self.h, _ptr(x), B, L, (ctypes.c_int * B)(*lengths), (ctypes.c_int * B)(*cut_bins), _ptr(y),
                                             self._stream()), "vfx_stft_lowpass")
        return y[0] if squeeze else y

    def stft_splice(self, x, y, cut_bins, lengths=None, ramp=0, gains=None):
        """The splice of restored clips onto their band-limited inputs in ONE launch (vfx_stft_splice): x (the input), y (the restored
        clip) (B, L) or (L,), pair b = the first lengths[b] samples of row b of both (default L; 1024 < lengths[b] <= L); cut_bins: the
        first bin that is y's alone, one int or one per clip (>= 0); ramp: the bins below it over which the weight of x falls from 1 to
        0 (splice.ramp_weights; 0: the hard mask of stft_lowpass); gains: g, one float or one per clip (default 1).  -> float32 of the
        same shape on the device, g y + ISTFT(a . STFT(x - g y)): x below the seam, g y above it; rows zero past their length.  Row b
        is bit for bit the chain stft -> weights -> istft on the pair alone, whatever batch it is in."""
        x, y = _dev_f32(x, self.device), _dev_f32(y, self.device)
        if x.dim() not in (1, 2) or x.shape != y.shape:
            raise ValueError("stft_splice: x %s and y %s must be equal (B, L) or (L,) tensors" % (tuple(x.shape), tuple(y.shape)))
        x, squeeze, B, L, lengths = _clip_rows(x, lengths, "stft_splice")
        y = y[None] if squeeze else y
        cut_bins = _per_clip(cut_bins, B, int, "stft_splice", "cut-off bins")
        if B == 0:
            raise ValueError("stft_splice: %d cut-off bins for %d clips" % (len(cut_bins), B))
        g = None if gains is None else (ctypes.c_float * B)(*_per_clip(gains, B, float, "stft_splice", "gains"))
        out = torch.empty((B, L), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_stft_splice(self.h, _ptr(x), _ptr(y), B, L, (ctypes.c_int * B)(*lengths), (ctypes.c_int * B)(*cut_bins),
                                            int(ramp), g, _ptr(out), self._stream()), "vfx_stft_splice")
        return out[0] if squeeze else out

    def band_power(self, a, b, lo_bins, hi_bins, lengths=None):
        """The power of two clips in a band of STFT bins (vfx_band_power): a, b (B, L) or (L,), pair p = the first lengths[p] samples of
        row p of both (default L; 1024 < lengths[p] <= L); lo_bins, hi_bins: the band lo <= k < hi, one int or one per clip
        (0 <= lo <= hi <= 1025) -> (B, 2) or (2,) float64 on the device: the sums over the clip's frames and the band of |A|^2 and
        |B|^2, the magnitudes stft's (eps 1e-8).  hi == lo gives zeros.  A pair's numbers do not depend on the batch it is in."""
        a, b = _dev_f32(a, self.device), _dev_f32(b, self.device)
        if a.dim() not in (1, 2) or a.shape != b.shape:
            raise ValueError("band_power: a %s and b %s must be equal (B, L) or (L,) tensors" % (tuple(a.shape), tuple(b.shape)))
        a, squeeze, B, L, lengths = _clip_rows(a, lengths, "band_power")
        b = b[None] if squeeze else b
        lo_bins = _per_clip(lo_bins, B, int, "band_power", "lower bins")
        hi_bins = _per_clip(hi_bins, B, int, "band_power", "upper bins")
        if B == 0:
            raise ValueError("band_power: no clips")
        out = torch.empty((B, 2), device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_band_power(self.h, _ptr(a), _ptr(b), B, L, (ctypes.c_int * B)(*lengths), (ctypes.c_int * B)(*lo_bins),
                                           (ctypes.c_int * B)(*hi_bins), _ptr(out), self._stream()), "vfx_band_power")
        return out[0] if squeeze else out

    def band_energy(self, wav, lengths=None, hop=512, threshold=0.95):
        """The bandwidth detector of load_wav_energy (tools/utils.py:33-44) for a padded batch (vfx_band_energy): wav (B, L) or (L,),
        clip b = the first lengths[b] samples of row b (default L; 1024 < lengths[b] <= L), 1 <= hop <= 2048 (librosa.stft's default
        512), 0 < threshold <= 1 -> (energy (B, 1025) float64: e[k] = sum_t log10(|STFT[k, t]| + 1), cut_bin (B,) int32: the first bin
        at which the exclusive prefix sum of e reaches threshold * (the sum of e[:1024])), both on the device.  A clip's numbers do not
        depend on the batch it is in nor on what the row holds past its end; an all-zero clip gives zeros and bin 0."""
        wav = _dev_f32(wav, self.device)
        if wav.dim() not in (1, 2):
            raise ValueError("band_energy: wav must be (B, L) or (L,), got %s" % (tuple(wav.shape),))
        wav, _, B, L, lengths = _clip_rows(wav, lengths, "band_energy")
        energy = torch.empty((B, _lib.BAND_BINS), device=self.device, dtype=torch.float64)
        cut_bin = torch.empty((B,), device=self.device, dtype=torch.int32)
        _lib.check(self.lib.vfx_band_energy(self.h, _ptr(wav), B, L, (ctypes.c_int * max(B, 1))(*lengths), int(hop), float(threshold),
                                            _ptr(energy), _ptr(cut_bin), self._stream()), "vfx_band_energy")
        return energy, cut_bin

    def band_cutoff(self, wav, lengths=None, sample_rate=44100, hop=512, threshold=0.95):
        """load_wav_energy's cut-off of every clip of a padded batch, in Hz: int((sample_rate // 2) * (cut_bin / 1025)), the reference's
        expression (tools/utils.py:44), evaluated on the host from Engine.band_energy's bins after ONE device-to-host copy."""
        wav = _dev_f32(wav, self.device)
        if wav.dim() not in (1, 2):
            raise ValueError("band_cutoff: wav must be (B, L) or (L,), got %s" % (tuple(wav.shape),))
        wav, _, B, L, lengths = _clip_rows(wav, lengths, "band_cutoff")
        cut_bin = torch.empty((B,), device=self.device, dtype=torch.int32)
        _lib.check(self.lib.vfx_band_energy(self.h, _ptr(wav), B, L, (ctypes.c_int * max(B, 1))(*lengths), int(hop), float(threshold),
                                            None, _ptr(cut_bin), self._stream()), "vfx_band_energy")
        return [int((int(sample_rate) // 2) * (i / _lib.BAND_BINS)) for i in cut_bin.cpu().tolist()]

    # ------------------------------------------------------------------ silence and activity (tools/others/audio_op.py:79-150)
    def _activity_rows(self, x, lengths, name):
        x, squeeze, B, L, lengths = _clip_rows(_float_rows(x, self.device, name, ValueError), lengths, name)
        if B == 0:
            raise ValueError("%s: no clips" % name)
        return x, B, L, (ctypes.c_int64 * B)(*lengths)

    def trim_bounds(self, x, lengths=None, threshold=500, sample_rate=44100, frame_length=0.02, which="both"):
        """trim_tail_empty (which="tail"), trim_head_empty ("head") or trim_empty ("both") of every clip of a padded batch as sample
        ranges (vfx_trim_bounds): x (B, L) or (L,), float32 or float64, clip b = the first lengths[b] samples (default L; 0 is
        allowed) of row b -> (start, stop), two (B,) int64 device tensors: the function keeps clip[start:stop], and start = stop = -1
        where it returns None.  The threshold is compared in x's dtype; a clip's bounds do not depend on the batch nor on what the row
        holds past its end.  activity.trim_empty is the host form."""
        x, B, L, lens = self._activity_rows(x, lengths, "trim_bounds")
        mode = {"tail": _lib.TRIM_TAIL, "head": _lib.TRIM_HEAD, "both": _lib.TRIM_BOTH}.get(which)
        if mode is None:
            raise ValueError("trim_bounds: which must be 'tail', 'head' or 'both', got %r" % (which,))
        start = torch.empty((B,), device=self.device, dtype=torch.int64)
        stop = torch.empty((B,), device=self.device, dtype=torch.int64)
        _lib.check(self.lib.vfx_trim_bounds(self.h, _ptr(x), int(x.dtype == torch.float64), B, L, lens, int(sample_rate * frame_length),
                                            float(threshold), mode, _ptr(start), _ptr(stop), self._stream()), "vfx_trim_bounds")
        return start, stop

    def has_long_empty(self, x, lengths=None, length=3, sample_rate=44100, threshold=400):
        """has_long_empty of every clip of a padded batch (vfx_long_empty): x and lengths as in `trim_bounds` -> (B,) int32 device
        tensor, 1 where a window of int(sample_rate * length) samples that ends at n, n - sample_rate, ... has a peak < threshold."""
        x, B, L, lens = self._activity_rows(x, lengths, "has_long_empty")
        flag = torch.empty((B,), device=self.device, dtype=torch.int32)
        _lib.check(self.lib.vfx_long_empty(self.h, _ptr(x), int(x.dtype == torch.float64), B, L, lens, int(sample_rate * length),
                                           int(sample_rate), float(threshold), _ptr(flag), self._stream()), "vfx_long_empty")
        return flag

    def active_frames_count(self, n, sample_rate=44100, frame_length=0.02, frame_shift=0.01):
        """The number of labels get_all_active_segment_index gives a clip of n samples (vfx_active_frames_count)."""
        return int(self.lib.vfx_active_frames_count(int(n), int(frame_length * sample_rate), int(frame_shift * sample_rate)))

    def active_frames(self, x, lengths=None, threshold=500, sample_rate=44100, frame_length=0.02, frame_shift=0.01):
        """get_all_active_segment_index of every clip of a padded batch (vfx_active_frames): x and lengths as in `trim_bounds`, every
        clip longer than int(frame_shift * sample_rate) samples -> (labels (B, F) uint8, counts (B,) int64), both on the device:
        labels[b, :counts[b]] are the clip's labels, 1 where the frame's peak > threshold; the rest of the row is 0."""
        x, B, L, lens = self._activity_rows(x, lengths, "active_frames")
        frame, shift = int(frame_length * sample_rate), int(frame_shift * sample_rate)
        ldf = max(1, max(int(self.lib.vfx_active_frames_count(int(n), frame, shift)) for n in lens))
        labels = torch.empty((B, ldf), device=self.device, dtype=torch.uint8)
        counts = torch.empty((B,), device=self.device, dtype=torch.int64)
        _lib.check(self.lib.vfx_active_frames(self.h, _ptr(x), int(x.dtype == torch.float64), B, L, lens, frame, shift, float(threshold),
                                              _ptr(labels), ldf, _ptr(counts), self._stream()), "vfx_active_frames")
        return labels, counts

    def spectral_metrics(self, est, target):
        """Per-clip (LSD, SiSpec dB) of est vs target, (B, T, F) or (B, 1, T, F) each -> (B, 2)."""
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        assert est.shape == target.shape
        F = est.shape[-1]
        T = est.shape[-2]
        B = est.numel() // (T * F)
        out = torch.empty((B, 2), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_spectral_metrics(self.h, _ptr(est), _ptr(target), B, T, F, _ptr(out), self._stream()),
                   "vfx_spectral_metrics")
        return out

    score_rates = (44100, 16000)   # the rates audio_metrics takes: the reference's two front ends (evaluation_proc/metrics.py:37-51)

    def _score_tables(self, rate):
        """Before the first call at 16 kHz: hand the library the reference's float32 evaluation of MelScale(80, 16000, 372) -- what
        set_mel_filterbank is to the 44.1 kHz table.  (Not through load_state_dict: the strict twin's state stays the models'.)"""
        if int(rate) == 16000 and not self._score16k_fb:
            from .models import MelScale
            fb = np.ascontiguousarray(MelScale.filterbank(372, 80, 16000, 8000.0).numpy(), dtype=np.float32)
            _lib.check(self.lib.vfx_load_tensor(self.h, MODEL_FRONTEND, b"mel16k.fb", fb.ctypes.data_as(ctypes.c_void_p),
                                                (ctypes.c_int64 * 2)(*fb.shape), 2), "vfx_load_tensor(mel16k.fb)")
            _lib.check(self.lib.vfx_finalize_weights(self.h, MODEL_FRONTEND), "vfx_finalize_weights")
            self._score16k_fb = True

    def audio_metrics(self, est, target, lengths=None, rate=44100):
        """AudioMetrics.evaluation's nine scores (metrics.METRIC_KEYS order) of waveform pairs at `rate` Hz (one of score_rates): est,
        target (B, L) or (L,), pair b = the first lengths[b] samples of row b (default: all L; 2646 <= lengths[b] <= L at 44.1 kHz,
        961 at 16 kHz) -> (B, 9) float64 on the device (vfx_audio_metrics_rate; at 44.1 kHz vfx_audio_metrics, bit for bit)."""
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        if est.dim() == 1:
            est, target = est[None], target[None]
        if est.shape != target.shape or est.dim() != 2:
            raise ValueError("audio_metrics: est %s and target %s must be equal (B, L) tensors" % (tuple(est.shape), tuple(target.shape)))
        est, _, B, L, lengths = _clip_rows(est, lengths, "audio_metrics")
        out = torch.empty((B, _lib.N_AUDIO_METRICS), device=self.device, dtype=torch.float64)
        self._score_tables(rate)
        _lib.check(self.lib.vfx_audio_metrics_rate(self.h, _ptr(est), _ptr(target), B, L, (ctypes.c_int * B)(*lengths), int(rate),
                                                   _ptr(out), self._stream()), "vfx_audio_metrics")
        return out

    STOI_RATE = 10000
    _STOI_MAX_HOST_TAPS = 1 << 20   # a longer filter is not built on the host: vfx_stoi refuses its tap count by itself

    def stoi_taps(self, fs):
        """(up, down, taps, ntaps) of `stoi` for clips at `fs` Hz: up / down = 10000 / fs reduced, taps = up * h / sum(h) of Octave's
        `resample` filter h (fc = 1 / (2 max(up, down)), roll-off fc / 10, 60 dB: a Kaiser-windowed sinc of 2 L + 1 taps), built in
        float64 on the host and cached on the device per (up, down).  taps is None at 10 kHz, and for a filter too long to build
        (vfx_stoi then refuses the tap count)."""
        fs = int(fs)
        if fs <= 0:
            raise ValueError("stoi: fs must be positive, got %d" % fs)
        g = math.gcd(self.STOI_RATE, fs)
        up, down = self.STOI_RATE // g, fs // g
        if up == down:
            return up, down, None, 0
        fc = 1.0 / (2 * max(up, down))
        L = int(math.ceil((60.0 - 8.0) / (28.714 * (fc / 10.0))))
        ntaps = 2 * L + 1
        if ntaps > self._STOI_MAX_HOST_TAPS:
            return up, down, None, min(ntaps, 2 ** 31 - 1)
        taps = self._stoi_taps.get((up, down))
        if taps is None:
            t = np.arange(-L, L + 1)
            h = np.kaiser(ntaps, 0.1102 * (60.0 - 8.7)) * (2 * up * fc * np.sinc(2 * fc * t))
            taps = torch.from_numpy(up * (h / np.sum(h))).to(self.device)
            self._stoi_taps[(up, down)] = taps
        return up, down, taps, ntaps

    def stoi(self, est, target, lengths=None, fs=44100):
        """STOI (Taal et al. 2011, as pystoi's stoi(target, est, fs, extended=False)) of waveform pairs at `fs` Hz: est, target (B, L)
        or (L,), pair b = the first lengths[b] samples of row b (default: all L) -> (B,) float64 on the device (vfx_stoi).  target is
        the clean signal; the score is not symmetric.  A pair with fewer than 30 frames left after the silent-frame removal scores
        1e-5.  A rate the resampling kernel does not take raises RuntimeError with the library's text."""
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        if est.dim() == 1:
            est, target = est[None], target[None]
        if est.shape != target.shape or est.dim() != 2:
            raise ValueError("stoi: est %s and target %s must be equal (B, L) tensors" % (tuple(est.shape), tuple(target.shape)))
        est, _, B, L, lengths = _clip_rows(est, lengths, "stoi")
        up, down, taps, ntaps = self.stoi_taps(fs)
        out = torch.empty(B, device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_stoi(self.h, _ptr(est), _ptr(target), B, L, (ctypes.c_int * max(B, 1))(*lengths), up, down,
                                     _ptr(taps) if taps is not None else None, ntaps, _ptr(out), self._stream()), "vfx_stoi")
        return out

    BSSEVAL_SLAB = _lib.BSSEVAL_SLAB   # samples per partial sum of vfx_bsseval: the slabs are cut from each clip's own extent

    def bsseval(self, est, target, lengths=None, flen=512):
        """BSS Eval v4 "images" SDR, ISR and SAR (Vincent et al. 2006; one source, one channel, one window over the whole file; restated
        from the definition in include/vfx.h, not pinned against museval) of waveform pairs: est, target (B, L) or (L,), pair b = the
        first lengths[b] samples of row b (default: all L) -> (B, 3) float64 on the device: sdr, isr, sar (vfx_bsseval).  flen: the taps
        of the distortion filter, a multiple of 16 in [16, 512].  A silent est or target scores NaN x 3; a denominator that is exactly
        zero gives +inf.  A flen or a length the library does not take raises RuntimeError with its text."""
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        if est.dim() == 1:
            est, target = est[None], target[None]
        if est.shape != target.shape or est.dim() != 2:
            raise ValueError("bsseval: est %s and target %s must be equal (B, L) tensors" % (tuple(est.shape), tuple(target.shape)))
        est, _, B, L, lengths = _clip_rows(est, lengths, "bsseval")
        out = torch.empty(B, 3, device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_bsseval(self.h, _ptr(est), _ptr(target), B, L, (ctypes.c_int * max(B, 1))(*lengths), int(flen),
                                        _ptr(out), self._stream()), "vfx_bsseval")
        return out

    def chunk_gather(self, x, win, hop, lead, n_chunks):
        """F.unfold with zero padding: x (B, L) -> (B, n_chunks, win), chunk k = x[k*hop - lead : ... + win]."""
        x = _dev_f32(x, self.device)
        B, L = x.shape
        chunks = torch.empty((B, n_chunks, win), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_chunk_gather(self.h, _ptr(x), B, L, win, hop, lead, n_chunks, _ptr(chunks),
                                             self._stream()), "vfx_chunk_gather")
        return chunks

    def chunk_ola(self, frames, window, scale, hop, lead, length):
        """Synthesis window (or scale) + F.fold: frames (B, n_chunks, win) -> (B, length)."""
        frames = _dev_f32(frames, self.device)
        B, n_chunks, win = frames.shape
        if window is not None:
            window = _dev_f32(window, self.device)
            assert window.numel() == win
        y = torch.empty((B, length), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_chunk_ola(self.h, _ptr(frames), _ptr(window) if window is not None else None,
                                          float(scale), B, n_chunks, win, hop, lead, length, _ptr(y),
                                          self._stream()), "vfx_chunk_ola")
        return y

    # ------------------------------------------------------------------ streaming sessions (vfx_stream_*; streaming.py drives them)
    def stream_create(self, slots, mode, win, hop_or_margin, window, scale, capacity, out_capacity):
        """A session of `slots` streams -> its handle.  mode: _lib.STREAM_OLA (hop) or _lib.STREAM_BOXCAR (in_margin); window: (win,)
        or None for the factor `scale`."""
        if window is not None:
            window = _dev_f32(window, self.device)
            if window.numel() != win:
                raise ValueError("stream_create: the window has %d samples, window size is %d" % (window.numel(), win))
        st = ctypes.c_void_p()
        _lib.check(self.lib.vfx_stream_create(self.h, int(slots), int(mode), int(win), int(hop_or_margin), _ptr(window), float(scale),
                                              int(capacity), int(out_capacity), ctypes.byref(st)), "vfx_stream_create")
        return st

    def stream_destroy(self, st):
        _lib.check(self.lib.vfx_stream_destroy(st), "vfx_stream_destroy")

    def stream_open(self, st):
        slot = ctypes.c_int()
        _lib.check(self.lib.vfx_stream_open(st, ctypes.byref(slot)), "vfx_stream_open")
        return slot.value

    def stream_push(self, st, slots, counts, packed):
        """counts[i] samples for slots[i], one after the other in `packed` (1-D float32 on the device)."""
        n = len(slots)
        if packed is not None and (packed.dtype != torch.float32 or packed.device != self.device or not packed.is_contiguous()
                                   or packed.numel() < sum(counts)):
            raise ValueError("stream_push: packed must be a contiguous float32 tensor on %s with all %d samples" % (self.device, sum(counts)))
        _lib.check(self.lib.vfx_stream_push(st, n, (ctypes.c_int * max(n, 1))(*slots), (ctypes.c_int64 * max(n, 1))(*counts),
                                            _ptr(packed), self._stream()), "vfx_stream_push")

    def stream_close(self, st, slot):
        _lib.check(self.lib.vfx_stream_close(st, int(slot)), "vfx_stream_close")

    def stream_next(self, st, max_rows, chunks):
        """The due chunks into `chunks` (room for max_rows of the longest row) -> (rows, row_len); rows = 0: nothing is due."""
        rows, row_len = ctypes.c_int(), ctypes.c_int()
        _lib.check(self.lib.vfx_stream_next(st, int(max_rows), _ptr(chunks), ctypes.byref(rows), ctypes.byref(row_len),
                                            self._stream()), "vfx_stream_next")
        return rows.value, row_len.value

    def stream_put(self, st, frames):
        """frames: the network's output for the rows of the outstanding stream_next, contiguous float32 (rows, row_len)."""
        if frames is not None and (frames.dtype != torch.float32 or frames.device != self.device or not frames.is_contiguous()):
            raise ValueError("stream_put: frames must be a contiguous float32 tensor on %s" % self.device)
        _lib.check(self.lib.vfx_stream_put(st, _ptr(frames), self._stream()), "vfx_stream_put")

    def stream_available(self, st, slot):
        n = ctypes.c_int64()
        _lib.check(self.lib.vfx_stream_available(st, int(slot), ctypes.byref(n)), "vfx_stream_available")
        return n.value

    def stream_room(self, st, slot):
        """How many samples a push to the slot may hold now."""
        n = ctypes.c_int64()
        _lib.check(self.lib.vfx_stream_room(st, int(slot), ctypes.byref(n)), "vfx_stream_room")
        return n.value

    def stream_state(self, st, slot):
        """(fed, released) of the slot's stream."""
        fed, released = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self.lib.vfx_stream_state(st, int(slot), ctypes.byref(fed), ctypes.byref(released)), "vfx_stream_state")
        return fed.value, released.value

    def stream_pop(self, st, slots, max_counts):
        """Up to max_counts[i] released samples of slots[i] -> a list of 1-D device tensors (views of one packed buffer)."""
        n = len(slots)
        have = [min(int(m), self.stream_available(st, s)) for s, m in zip(slots, max_counts)]
        packed = torch.empty(max(sum(have), 1), device=self.device, dtype=torch.float32)
        got = (ctypes.c_int64 * max(n, 1))()
        _lib.check(self.lib.vfx_stream_pop(st, n, (ctypes.c_int * max(n, 1))(*slots), (ctypes.c_int64 * max(n, 1))(*have), _ptr(packed),
                                           got, self._stream()), "vfx_stream_pop")
        out, off = [], 0
        for i in range(n):
            out.append(packed[off:off + got[i]])
            off += got[i]
        return out

    # ------------------------------------------------------------------ resampling (librosa.load(path, sr) = scipy resample_poly)
    @staticmethod
    def resample_ratio(sr_in, sr_out):
        """(up, down) of resample_poly for sr_in -> sr_out, reduced by their gcd."""
        g = math.gcd(int(sr_in), int(sr_out))
        return int(sr_out) // g, int(sr_in) // g

    @staticmethod
    def resample_out_len(n_in, sr_in, sr_out):
        """len(resample_poly(x[:n_in], up, down)) = ceil(n_in * up / down); -1 for a pair the kernel does not take."""
        up, down = Engine.resample_ratio(sr_in, sr_out)
        return int(_lib.load().vfx_resample_out_len(int(n_in), up, down))

    @staticmethod
    def resample_supported(sr_in, sr_out):
        """True when `resample` takes sr_in -> sr_out on the device (the same rate included)."""
        return int(sr_in) > 0 and int(sr_out) > 0 and Engine.resample_out_len(1, sr_in, sr_out) >= 0

    @staticmethod
    def resample_window(n_in, sr_in, sr_out, o0, n):
        """The input indices [k0, k1) that outputs [o0, o0 + n) of a clip of n_in samples read (vfx_resample_window): what the
        window form of `resample` must be handed.  (0, 0) when none is (outputs past the clip's end are zeros)."""
        up, down = Engine.resample_ratio(sr_in, sr_out)
        k0, k1 = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.load().vfx_resample_window(int(n_in), up, down, int(o0), int(n), ctypes.byref(k0), ctypes.byref(k1)),
                   "vfx_resample_window")
        return k0.value, k1.value

    def resample_taps(self, sr_in, sr_out):
        """The float32 taps resample_poly builds for the pair (scipy's own firwin call), cached on the device per (up, down)."""
        key = self.resample_ratio(sr_in, sr_out)
        taps = self._resample_taps.get(key)
        if taps is None:
            from scipy.signal import firwin
            up, down = key
            m = max(up, down)
            h = firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32)
            h *= up                                  # in float32, as resample_poly does
            taps = torch.from_numpy(h).to(self.device)
            self._resample_taps[key] = taps
        return taps

    def resample(self, x, sr_in, sr_out, lengths=None, x0=0, o0=0, n_out=None):
        """scipy.signal.resample_poly(x, up, down) of float32 clips on the device, bit for bit: x (B, L) or (L,) -> (y, out_lengths).

        lengths: each clip's true length (default: x0 + L); samples past it count as zero, and y is zero at or past a clip's output
        length out_lengths[b] = ceil(lengths[b] * up / down).  Window form (streamed input): x holds input indices [x0, x0 + L) of
        every clip, and y (B, n_out) receives outputs [o0, o0 + n_out) (default: up to the longest clip's output length); the window
        must hold what `resample_window` asks for, or the call raises.  1-D x gives a 1-D y and an int out length."""
        x0, o0 = int(x0), int(o0)
        x, squeeze, B, L, lens = _clip_rows(_dev_f32(x, self.device), lengths, "resample")
        lengths = [x0 + L] * B if lengths is None else lens
        up, down = self.resample_ratio(sr_in, sr_out)
        out_lengths = [self.resample_out_len(n, sr_in, sr_out) for n in lengths]
        if any(n < 0 for n in out_lengths):
            raise RuntimeError("resample: %d Hz -> %d Hz is not supported on the device (its filter does not fit the kernel)"
                               % (sr_in, sr_out))
        if n_out is None:
            n_out = max(0, max(out_lengths) - o0)
        if up == down:      # the same rate: resample_poly returns a copy
            y = torch.zeros((B, int(n_out)), device=self.device, dtype=torch.float32)
            for b in range(B):
                k0, k1 = self.resample_window(lengths[b], sr_in, sr_out, o0, n_out)
                if k1 > k0:
                    if k0 < x0 or k1 > x0 + L:
                        raise RuntimeError("resample: the window [%d, %d) lacks samples [%d, %d)" % (x0, x0 + L, k0, k1))
                    y[b, k0 - o0:k1 - o0] = x[b, k0 - x0:k1 - x0]
        else:               # (the kernel writes every element of y: zeros at or past a clip's output length)
            y = torch.empty((B, int(n_out)), device=self.device, dtype=torch.float32)
            if n_out > 0:
                taps = self.resample_taps(sr_in, sr_out)
                lens = (ctypes.c_int64 * B)(*lengths)
                _lib.check(self.lib.vfx_resample(self.h, _ptr(x), B, L, x0, L, lens, up, down, _ptr(taps), taps.numel(), _ptr(y),
                                                 int(n_out), o0, int(n_out), self._stream()), "vfx_resample")
        return (y[0], out_lengths[0]) if squeeze else (y, out_lengths)

    # ------------------------------------------------------------------ resampling with a rate pair per clip (the "stft" low-pass)
    MAX_RESAMPLE_EACH_CLIPS = 128
    RESAMPLE_EACH_CACHE_BYTES = 256 << 20

    @staticmethod
    def resample_each_out_len(n_in, sr_in, sr_out):
        """len(resample_poly(x[:n_in], up, down)); -1 for a pair past `resample_each`'s cap (vfx_resample_each_out_len)."""
        up, down = Engine.resample_ratio(sr_in, sr_out)
        if not (0 < up < 1 << 31 and 0 < down < 1 << 31):
            return -1
        return int(_lib.load().vfx_resample_each_out_len(int(n_in), up, down))

    @staticmethod
    def resample_each_supported(sr_in, sr_out):
        """True when `resample_each` takes sr_in -> sr_out: both rates positive and max(up, down) <= 65536 after the gcd."""
        return int(sr_in) > 0 and int(sr_out) > 0 and Engine.resample_each_out_len(1, sr_in, sr_out) >= 0

    def _resample_each_taps(self, ms, dtype):
        """The unscaled filters of resample_poly for the rates `ms` (M = max(up, down)): firwin(20 M + 1, 1 / M, ("kaiser", 5.0)) from
        SciPy on the host, in `dtype`, cached on the device per (M, dtype) -- the down and the up step of a cut-off share one.  The
        cache is bounded: past RESAMPLE_EACH_CACHE_BYTES (256 MiB) the least recently used designs go, never one of `ms`.
        -> (one device tensor holding the filters of `ms` back to back, {M: its first element})."""
        cache = self._resample_each_cache
        np_dtype = np.float32 if dtype == torch.float32 else np.float64
        for m in ms:
            key = (m, dtype)
            if key in cache:
                cache.move_to_end(key)
            else:
                from scipy.signal import firwin
                cache[key] = torch.from_numpy(firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np_dtype)).to(self.device)
        needed = {(m, dtype) for m in ms}
        total = sum(t.numel() * t.element_size() for t in cache.values())
        for key in [k for k in cache if k not in needed]:      # oldest first
            if total <= self.RESAMPLE_EACH_CACHE_BYTES:
                break
            t = cache.pop(key)
            total -= t.numel() * t.element_size()
        parts = [cache[(m, dtype)] for m in ms]
        at, n = {}, 0
        for m, t in zip(ms, parts):
            at[m] = n
            n += t.numel()
        if not parts:
            return torch.zeros(1, device=self.device, dtype=dtype), at
        return (parts[0] if len(parts) == 1 else torch.cat(parts)), at

    def resample_each(self, x, sr_in, sr_out, lengths=None, n_out=None, _y=None):
        """scipy.signal.resample_poly(clip b, up_b, down_b) with a rate pair per clip, on the device, bit for bit, in the clips' dtype:
        x (B, L) or (L,), float32 or float64 (any other dtype raises TypeError: SciPy treats integer input differently, which stays
        with the caller) -> (y, out_lengths), y of x's dtype.

        sr_in / sr_out: each an int or one int per clip; any pair with max(up, down) <= 65536 after the gcd (`resample_each_supported`;
        RuntimeError naming the clip and its pair otherwise), the same rate included (a copy).  lengths: each clip's true length
        (default L).  y (B, n_out) -- n_out defaults to the longest output -- holds row b's first n_out outputs, zeros at or past
        out_lengths[b] = ceil(lengths[b] up_b / down_b).  The distinct reduced pairs of a call are its designs; B > 128 is cut into
        calls of 128.  The unscaled filters come from SciPy's firwin on the host and are cached on the device per (M, dtype), least
        recently used evicted past RESAMPLE_EACH_CACHE_BYTES = 256 MiB (`_resample_each_taps`).  1-D x gives a 1-D y and an int."""
        x, squeeze, B, L, lengths = _clip_rows(_float_rows(x, self.device, "resample_each", TypeError), lengths, "resample_each")
        if B and (min(lengths) < 0 or max(lengths) > L):
            raise ValueError("resample_each: clips of %d .. %d samples in rows of %d" % (min(lengths), max(lengths), L))
        sr_in, sr_out = _per_clip(sr_in, B, int, "resample_each", "sr_in"), _per_clip(sr_out, B, int, "resample_each", "sr_out")
        for rates, what in ((sr_in, "sr_in"), (sr_out, "sr_out")):
            if any(r <= 0 for r in rates):
                raise ValueError("resample_each: %s must be positive" % what)
        pairs = [self.resample_ratio(i, o) for i, o in zip(sr_in, sr_out)]
        for b, (up, down) in enumerate(pairs):
            if max(up, down) > 65536:
                raise RuntimeError("resample_each: clip %d: %d Hz -> %d Hz is the pair %d/%d, past the cap max(up, down) <= 65536"
                                   % (b, sr_in[b], sr_out[b], up, down))
        out_lengths = [-((-n * up) // down) for n, (up, down) in zip(lengths, pairs)]
        n_out = max(out_lengths, default=0) if n_out is None else int(n_out)
        if n_out < 0:
            raise ValueError("resample_each: n_out = %d" % n_out)
        y = _result_rows(_y, (B, n_out), x.dtype, x.device, "resample_each")
        if L == 0:
            y.zero_()
        for b0 in range(0, B if n_out and L else 0, self.MAX_RESAMPLE_EACH_CLIPS):
            chunk = pairs[b0:b0 + self.MAX_RESAMPLE_EACH_CLIPS]
            designs = sorted(set(chunk))
            taps, at = self._resample_each_taps(sorted({max(p) for p in designs if p[0] != p[1]}), x.dtype)
            nb, F = len(chunk), len(designs)
            _lib.check(self.lib.vfx_resample_each(
                self.h, _ptr(x[b0:]), int(x.dtype == torch.float64), nb, L, (ctypes.c_int64 * nb)(*lengths[b0:b0 + nb]),
                (ctypes.c_int * nb)(*[designs.index(p) for p in chunk]), (ctypes.c_int * F)(*[p[0] for p in designs]),
                (ctypes.c_int * F)(*[p[1] for p in designs]), _ptr(taps),
                (ctypes.c_int64 * F)(*[at.get(max(p), 0) if p[0] != p[1] else 0 for p in designs]), F, _ptr(y[b0:]), n_out, n_out,
                self._stream()), "vfx_resample_each")
        return (y[0], out_lengths[0]) if squeeze else (y, out_lengths)

    # ------------------------------------------------------------------ zero-phase IIR filter (scipy.signal.sosfiltfilt)
    MAX_SOS_SECTIONS = 16

    @staticmethod
    def _check_sos(sos):
        """sos as SciPy validates it (its wording), float64 (S, 6) C-contiguous."""
        sos = np.ascontiguousarray(np.atleast_2d(np.asarray(sos)), dtype=np.float64)
        if sos.ndim != 2:
            raise ValueError("sos array must be 2D")
        if sos.shape[1] != 6:
            raise ValueError("sos array must be shape (n_sections, 6)")
        if not (sos[:, 3] == 1).all():
            raise ValueError("sos[:, 3] should be all ones")
        if not 1 <= sos.shape[0] <= Engine.MAX_SOS_SECTIONS:
            raise ValueError("sosfiltfilt: %d sections, the device filter takes 1 .. %d" % (sos.shape[0], Engine.MAX_SOS_SECTIONS))
        return sos

    @staticmethod
    def sosfiltfilt_padlen(sos):
        """The default padlen of scipy.signal.sosfiltfilt(sos, x): 3 * (2 S + 1 - min(#{b2 == 0}, #{a2 == 0}))."""
        sos = Engine._check_sos(sos)
        ntaps = 2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
        return 3 * ntaps

    def sosfiltfilt(self, x, sos, lengths=None):
        """scipy.signal.sosfiltfilt(sos, x) of every clip on the device, bit for bit: x (B, L) or (L,), float32 or float64 (any other
        dtype is converted to float64 first; SciPy extends an integer clip in its own dtype, where the extension can wrap) -> float64 tensor of the same shape.  lengths: each clip's true length (default L);
        a row is zero past it.  ValueError, with SciPy's wording, for a clip that is not longer than padlen and for a malformed sos."""
        sos = self._check_sos(sos)
        padlen = self.sosfiltfilt_padlen(sos)
        x, squeeze, B, L, lengths = _clip_rows(_float_rows(x, self.device, "sosfiltfilt", torch.float64), lengths, "sosfiltfilt")
        if B == 0 or min(lengths) <= padlen:
            raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
        if max(lengths) > L:
            raise ValueError("sosfiltfilt: a clip of %d samples in rows of %d" % (max(lengths), L))
        from scipy.signal import sosfilt_zi
        zi = np.ascontiguousarray(sosfilt_zi(sos), dtype=np.float64)
        y = torch.empty((B, L), device=self.device, dtype=torch.float64)
        dbl = ctypes.POINTER(ctypes.c_double)
        lens = (ctypes.c_int64 * B)(*lengths)
        _lib.check(self.lib.vfx_sosfiltfilt(self.h, _ptr(x), int(x.dtype == torch.float64), B, L, lens, sos.ctypes.data_as(dbl),
                                            sos.shape[0], zi.ctypes.data_as(dbl), padlen, _ptr(y), L, self._stream()),
                   "vfx_sosfiltfilt")
        return y[0] if squeeze else y

    MAX_SOS_DESIGNS = 128

    def sosfiltfilt_bank(self, x, bank, filter_index=None, lengths=None):
        """`sosfiltfilt` with a design per clip: row b is scipy.signal.sosfiltfilt(bank[filter_index[b]], clip b), bit for bit.
        bank: a list of (S_f, 6) arrays, of any mixture of section counts (1 .. 16; at most 128 designs); filter_index: one index
        per clip (default clip b takes design b, which needs len(bank) == B).  x, lengths and the result as in `sosfiltfilt`.  One
        pair of launches takes the whole batch whatever its section counts.  ValueError, with SciPy's wording, for a malformed
        design and for a clip that is not longer than ITS design's padlen (the message carries that padlen)."""
        bank = [self._check_sos(sos) for sos in bank]
        x, squeeze, B, L, lengths = _clip_rows(_float_rows(x, self.device, "sosfiltfilt_bank", torch.float64), lengths,
                                               "sosfiltfilt_bank")
        F = len(bank)
        if B == 0 or not 1 <= F <= self.MAX_SOS_DESIGNS:
            raise ValueError("sosfiltfilt_bank: %d clips and %d designs (at most %d)" % (B, F, self.MAX_SOS_DESIGNS))
        if filter_index is None:
            if F != B:
                raise ValueError("sosfiltfilt_bank: %d designs for %d clips and no filter_index" % (F, B))
            filter_index = range(B)
        filter_index = [int(v) for v in filter_index]
        if len(filter_index) != B or any(not 0 <= f < F for f in filter_index):
            raise ValueError("sosfiltfilt_bank: %d indices for %d clips, each must be in [0, %d)" % (len(filter_index), B, F))
        padlens = [self.sosfiltfilt_padlen(sos) for sos in bank]
        for n, f in zip(lengths, filter_index):
            if n <= padlens[f]:
                raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlens[f])
        if max(lengths) > L:
            raise ValueError("sosfiltfilt_bank: a clip of %d samples in rows of %d" % (max(lengths), L))
        from scipy.signal import sosfilt_zi
        sections = [sos.shape[0] for sos in bank]
        Smax = max(sections)
        sos_all = np.zeros((F, Smax, 6), dtype=np.float64)
        zi_all = np.zeros((F, Smax, 2), dtype=np.float64)
        for f, sos in enumerate(bank):
            sos_all[f, :sections[f]] = sos
            zi_all[f, :sections[f]] = sosfilt_zi(sos)
        y = torch.empty((B, L), device=self.device, dtype=torch.float64)
        dbl = ctypes.POINTER(ctypes.c_double)
        _lib.check(self.lib.vfx_sosfiltfilt_bank(self.h, _ptr(x), int(x.dtype == torch.float64), B, L, (ctypes.c_int64 * B)(*lengths),
                                                 (ctypes.c_int * B)(*filter_index), sos_all.ctypes.data_as(dbl),
                                                 zi_all.ctypes.data_as(dbl), (ctypes.c_int * F)(*sections), (ctypes.c_int * F)(*padlens),
                                                 F, Smax, _ptr(y), L, self._stream()), "vfx_sosfiltfilt_bank")
        return y[0] if squeeze else y

    # ------------------------------------------------------------------ room-impulse-response convolution (MagicalEffects.reverb_rir)
    MAX_RIR_TAPS = 1 << 20

    def reverb_rir(self, x, rirs, rir_index=None, lengths=None, rir_lengths=None, normalize=True):
        """MagicalEffects.reverb_rir of float32 clips on the device: x (B, L) or (L,), rirs (R, M) or (M,) -> (y, peaks), both on the
        device.  Clip b is convolved with RIR rir_index[b] (default b % R) in direct form, over the full length; peaks[b] is the
        largest |sample| of that full convolution, tail included; with `normalize` a clip whose peak exceeds 0.99 is scaled to a
        peak of 0.98, as the reference does; y holds the first lengths[b] samples (default L) of each, zeros past them.
        rir_lengths: taps of each RIR (default M).  1-D x gives a 1-D y and a 0-D peak.  Per sample
        |y - exact| <= (min(taps, 1024) + 2) 2^-24 sum |x||h| + 2^-149, and a clip's result does not depend on the batch."""
        x = _dev_f32(x, self.device)
        rirs = _dev_f32(rirs, self.device)
        squeeze = x.dim() == 1
        if squeeze:
            x = x[None]
        if rirs.dim() == 1:
            rirs = rirs[None]
        if x.dim() != 2 or rirs.dim() != 2:
            raise ValueError("reverb_rir: x must be (B, L) or (L,) and rirs (R, M) or (M,), got %s and %s"
                             % (tuple(x.shape), tuple(rirs.shape)))
        x, _, B, L, lengths = _clip_rows(x, lengths)      # (the counts are checked together below)
        R, M = rirs.shape
        rir_lengths = [M] * R if rir_lengths is None else [int(v) for v in rir_lengths]
        if R == 0 or B == 0:
            raise ValueError("reverb_rir: %d clips and %d RIRs" % (B, R))
        rir_index = [b % R for b in range(B)] if rir_index is None else [int(v) for v in rir_index]
        if len(lengths) != B or len(rir_index) != B or len(rir_lengths) != R:
            raise ValueError("reverb_rir: %d lengths and %d indices for %d clips, %d lengths for %d RIRs"
                             % (len(lengths), len(rir_index), B, len(rir_lengths), R))
        y = torch.empty((B, L), device=self.device, dtype=torch.float32)
        peaks = torch.empty((B,), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_reverb_rir(self.h, _ptr(x), B, L, (ctypes.c_int64 * B)(*lengths), _ptr(rirs), R, M,
                                           (ctypes.c_int64 * R)(*rir_lengths), (ctypes.c_int * B)(*rir_index), int(bool(normalize)),
                                           _ptr(y), L, _ptr(peaks), self._stream()), "vfx_reverb_rir")
        return (y[0], peaks[0]) if squeeze else (y, peaks)

    # ------------------------------------------------------------------ noise mixing (add_noise_and_scale and its HQ / Aug forms)
    def mix_noise(self, front, noise, hq=None, aug=None, lengths=None, noise_weight=None, scale=None, want_noisy=False):
        """add_noise_and_scale (front, noise), add_noise_and_scale_with_HQ (+ hq) or add_noise_and_scale_with_HQ_with_Aug (+ hq, aug)
        of float32 clips on the device: every signal (B, L) or (L,), clip b = the first lengths[b] samples (default L) of row b of
        each; what the rows hold past them is not read.  noise_weight: 10 ** (snr / 20) per clip (a number: the same for every clip),
        None skips the SNR step; scale: the common scale per clip (default 1).  -> dict of device tensors shaped like `front`:
        "front", "noise", "hq" and "aug" where given, and "noisy" = noise + speech (front, or aug when given) when asked for; rows
        are zero past their length.  One float32 operation per sample and step, in the host functions' order: the plain form equals
        simulate.add_noise_and_scale bit for bit, and a clip's result does not depend on the batch."""
        sig = {"front": front, "noise": noise, "hq": hq, "aug": aug}
        sig = {k: _dev_f32(v, self.device) for k, v in sig.items() if v is not None}
        front = sig["front"]
        if any(v.shape != front.shape for v in sig.values()) or front.dim() not in (1, 2):
            raise ValueError("mix_noise: every signal must be (B, L) or (L,) of one shape, got %s"
                             % ", ".join("%s %s" % (k, tuple(v.shape)) for k, v in sig.items()))
        _, squeeze, B, L, lengths = _clip_rows(front, lengths)      # (the counts are checked together below)
        if squeeze:
            sig = {k: v[None] for k, v in sig.items()}
        if B == 0:
            raise ValueError("mix_noise: no clips")
        scale = _per_clip(1.0 if scale is None else scale, B, float)
        weight = None if noise_weight is None else _per_clip(noise_weight, B, float)
        if len(lengths) != B or len(scale) != B or (weight is not None and len(weight) != B):
            raise ValueError("mix_noise: %d lengths, %d scales and %s weights for %d clips"
                             % (len(lengths), len(scale), "no" if weight is None else len(weight), B))
        form = 2 if "aug" in sig else (1 if "hq" in sig else 0)      # (aug without hq: the library says so)
        out = {k: torch.empty((B, L), device=self.device, dtype=torch.float32) for k in sig}
        if want_noisy:
            out["noisy"] = torch.empty((B, L), device=self.device, dtype=torch.float32)
        dbl = ctypes.c_double * B
        _lib.check(self.lib.vfx_mix_noise(self.h, form, B, L, (ctypes.c_int64 * B)(*lengths), _ptr(sig["front"]), _ptr(sig["noise"]),
                                          _ptr(sig.get("hq")), _ptr(sig.get("aug")), dbl(*weight) if weight is not None else None,
                                          dbl(*scale), _ptr(out["front"]), _ptr(out["noise"]), _ptr(out.get("hq")),
                                          _ptr(out.get("aug")), _ptr(out.get("noisy")), self._stream()), "vfx_mix_noise")
        return {k: v[0] for k, v in out.items()} if squeeze else out

    # ------------------------------------------------------------------ array effects (MagicalEffects.quantification, time_dropout)
    MAX_QUANT_BINS = 16

    def quantize(self, x, bins, lengths=None, _y=None):
        """MagicalEffects.quantification of every clip on the device: x (B, L) or (L,), float32 or float64; bins one int for all or
        one per clip, each in 0..16; clip b = the first lengths[b] samples (default L) of row b, what the row holds past them is not
        read.  -> (y, peaks): y float64 shaped like x, zero past each length, bit for bit simulate.quantification; peaks (B,) in
        x's dtype (0-D for a 1-D x), max |x| of each clip.  A clip's result does not depend on the batch."""
        x, squeeze, B, L, lengths = _clip_rows(_float_rows(x, self.device, "quantize", ValueError), lengths, "quantize")
        if B == 0:
            raise ValueError("quantize: no clips")
        bins = _per_clip(bins, B, int, "quantize", "bins")
        y = _result_rows(_y, (B, L), torch.float64, x.device, "quantize")
        peaks = torch.empty((B,), device=x.device, dtype=x.dtype)
        _lib.check(self.lib.vfx_quantize(self.h, _ptr(x), int(x.dtype == torch.float64), B, L, (ctypes.c_int64 * B)(*lengths),
                                         (ctypes.c_int * B)(*bins), _ptr(y), L, _ptr(peaks), self._stream()), "vfx_quantize")
        return (y[0], peaks[0]) if squeeze else (y, peaks)

    def time_dropout(self, x, starts, ends, lengths=None, _y=None):
        """MagicalEffects.time_dropout of every clip on the device: x and lengths as in `quantize`; starts, ends: the sample range
        [start, end) to silence, one pair for all or one per clip, 0 <= start <= end (simulate.time_dropout's int(length * start)
        and int(length * start + length * trunk_length)).  -> tensor shaped like x in x's dtype, zero past each length: x with the
        range zeroed and the 96-sample patches of `smooth` around start and around end, each skipped when its centre is closer than
        50 samples to either end of the clip.  Outside the patches bit for bit the host function; inside, the 25-term float64 sum
        of simulate.smooth_matrix() rounded once."""
        from .simulate import smooth_matrix
        x, squeeze, B, L, lengths = _clip_rows(_float_rows(x, self.device, "time_dropout", ValueError), lengths, "time_dropout")
        if B == 0:
            raise ValueError("time_dropout: no clips")
        starts, ends = _per_clip(starts, B, int, "time_dropout", "starts"), _per_clip(ends, B, int, "time_dropout", "ends")
        y = _result_rows(_y, (B, L), x.dtype, x.device, "time_dropout")
        i64 = ctypes.c_int64 * B
        _lib.check(self.lib.vfx_time_dropout(self.h, _ptr(x), int(x.dtype == torch.float64), B, L, i64(*lengths), i64(*starts), i64(*ends),
                                             smooth_matrix().ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _ptr(y), L,
                                             self._stream()), "vfx_time_dropout")
        return y[0] if squeeze else y

    # ------------------------------------------------------------------ effect chain (the biquads, clip and reverse of the sox chain)
    MAX_CHAIN_OPS = 8
    MAX_CHAIN_STAGES = 4
    _CHAIN_OPS = {"biquad": 1, "clip": 2, "reverse": 3}

    @classmethod
    def effect_chain_supported(cls, program):
        """Whether `effect_chain` takes this program: known steps, at most 8 of them, at most 4 biquads between two clip steps."""
        if len(program) > cls.MAX_CHAIN_OPS or any(step[0] not in cls._CHAIN_OPS for step in program):
            return False
        run = 0
        for step in program:
            run = 0 if step[0] == "clip" else run + (step[0] == "biquad")
            if run > cls.MAX_CHAIN_STAGES:
                return False
        return True

    def effect_chain(self, x, programs, lengths=None):
        """The biquads, clip and reverse of MagicalEffects' sox chain on the device, a program per clip: x (B, L) or (L,), made
        float32; programs: one program for all, or one per clip, a program being a sequence of steps ("biquad", (b0, b1, b2, a1, a2))
        -- simulate.biquad_design's --, ("clip", factor) and ("reverse",), at most 8 of them with at most 4 biquads between two clip
        steps; clip b = the first lengths[b] samples (default L) of row b.  -> float32 tensor shaped like x, zero past each
        length, bit for bit simulate.chain_effects for a clip of finite samples; a clip's result does not depend on the batch."""
        x = _dev_f32(x, self.device)
        if x.dim() not in (1, 2):
            raise ValueError("effect_chain: x must be (B, L) or (L,), got %s" % (tuple(x.shape),))
        x, squeeze, B, L, lengths = _clip_rows(x, lengths, "effect_chain")
        if B == 0:
            raise ValueError("effect_chain: no clips")
        programs = list(programs)
        if all(len(step) > 0 and isinstance(step[0], str) for step in programs):      # one program (an empty one included) for all
            programs = [programs] * B
        if len(programs) != B:
            raise ValueError("effect_chain: %d programs for %d clips" % (len(programs), B))
        for b, program in enumerate(programs):
            if not self.effect_chain_supported(program):
                raise ValueError("effect_chain: clip %d: the device takes at most %d steps of %s with at most %d biquads between two "
                                 "clip steps, got %s" % (b, self.MAX_CHAIN_OPS, sorted(self._CHAIN_OPS), self.MAX_CHAIN_STAGES,
                                                         [step[0] for step in program]))
        K = max(1, max(len(p) for p in programs))
        ops = np.zeros((B, K), dtype=np.int32)
        coef = np.zeros((B, K, 5), dtype=np.float64)
        for b, program in enumerate(programs):
            for k, step in enumerate(program):
                ops[b, k] = self._CHAIN_OPS[step[0]]
                if step[0] == "biquad":
                    coef[b, k] = step[1]
                elif step[0] == "clip":
                    coef[b, k, 0] = step[1]
        y = torch.empty((B, L), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_effect_chain(self.h, _ptr(x), B, L, (ctypes.c_int64 * B)(*lengths),
                                             ops.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                             coef.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), K, _ptr(y), L, self._stream()),
                   "vfx_effect_chain")
        return y[0] if squeeze else y

    def resunet_mel(self, mel_linear):
        """Generator.forward: linear mel (B,T,128) -> log10 mel (B,T,128)."""
        mel = _dev_f32(mel_linear, self.device)
        B, T, _ = mel.shape
        out = torch.empty_like(mel)
        _lib.check(self.lib.vfx_resunet_mel(self.h, _ptr(mel), B, T, _ptr(out), self._stream()), "vfx_resunet_mel")
        return out

    def analysis_mel(self, model, mel_linear, frames=None):
        """Generator.forward with analysis module `model` (MODEL_UNET_MEL, MODEL_GRU_MEL or MODEL_DNN_MEL): linear mel (B,T,128)
        -> log10 mel estimate (B,T,128).  `frames` (B ints, or None = all T): clip b has frames[b] live rows; its result is that of
        its own call on them, rows past them are zero (the ResUNet takes None only)."""
        mel = _dev_f32(mel_linear, self.device)
        B, T, _ = mel.shape
        out = torch.empty_like(mel)
        arr = None
        if frames is not None:
            frames = _clip_rows(mel[:, :, 0], frames, "analysis_mel", "frame counts")[4]
            arr = (ctypes.c_int * B)(*frames)
        _lib.check(self.lib.vfx_analysis_mel(self.h, int(model), _ptr(mel), B, T, arr, _ptr(out), self._stream()),
                   "vfx_analysis_mel")
        return out

    def select_analysis(self, model):
        """The analysis module restore_gsr / restore_gsr_varlen run (default MODEL_UNET_MEL); its weights must be loaded."""
        _lib.check(self.lib.vfx_select_analysis(self.h, int(model)), "vfx_select_analysis")
        self.analysis_model = int(model)
        if self._strict is not None:
            self._strict.select_analysis(model)

    def resunet_spec(self, sp, wav):
        sp, wav = _dev_f32(sp, self.device), _dev_f32(wav, self.device)
        B, T, _ = sp.shape
        L = wav.shape[-1]
        out = torch.empty((B, L), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_resunet_spec(self.h, _ptr(sp), _ptr(wav), B, T, L, _ptr(out), self._stream()),
                   "vfx_resunet_spec")
        return out

    def vocoder_out_len(self, T):
        return int(self.lib.vfx_vocoder_out_len(self.h, T))

    def vocoder(self, mel_linear):
        mel = _dev_f32(mel_linear, self.device)
        B, T, _ = mel.shape
        out = torch.empty((B, self.vocoder_out_len(T)), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.vfx_vocoder(self.h, _ptr(mel), B, T, _ptr(out), self._stream()), "vfx_vocoder")
        return out

    def restore_gsr(self, wav, unify_energy=False, want_logmel=False, out=None):
        """Whole handler() segment body for a batch: wav (B, L) -> restored (B, L)."""
        wav = _dev_f32(wav, self.device)
        B, L = wav.shape
        if out is None:
            out = torch.empty_like(wav)
        logmel = torch.empty((B, self.frames(L), N_MELS), device=self.device, dtype=torch.float32) if want_logmel else None
        _lib.check(self.lib.vfx_restore_gsr(self.h, _ptr(wav), B, L, _ptr(out), _ptr(logmel), int(bool(unify_energy)),
                                            self._stream()), "vfx_restore_gsr")
        return (out, logmel) if want_logmel else out

    def padded_frames(self, L):
        """The ResUNet's padded frame count of a clip of L samples (unet.py:75-77): 64 * ceil(T / 64) -- the bucket key of
        restore_ssr_varlen, and the granule restore_gsr_varlen's callers pad a batch's row length to (one cached plan per row length)."""
        return -(-self.frames(L) // 64) * 64

    def supports_varlen(self):
        """False for the one configuration vfx_restore_gsr_varlen refuses: the 16-bit mode on the fp32 trunk (VFX_TUNE_F32_TRUNK, or
        a ResStack slope outside (0, 1]) -- the persistent C = 64 kernel has no register left for a clip's length there.  Callers
        that bucket clips (dist.checked_restore, VoiceFixer.restore_list) then batch EQUAL lengths only, as rounds 1-4 did."""
        if self.precision != 2:
            return True
        slope = float(self.cfg.voc_res_slope)
        return not (int(self.cfg.tuning) & _lib.TUNE_F32_TRUNK) and 0.0 < slope <= 1.0

    def _varlen_args(self, wav, lengths, out, name):
        """The prologue of the two varlen entries -> (wav on the device, B, Lmax, the lengths as the C int array, out)."""
        wav, _, B, L, lengths = _clip_rows(_dev_f32(wav, self.device), lengths, name)
        return wav, B, L, (ctypes.c_int * B)(*lengths), torch.empty_like(wav) if out is None else out

    def restore_gsr_varlen(self, wav, lengths, unify_energy=False, want_logmel=False, out=None):
        """The handler() segment body for a batch of clips of UNEQUAL length: wav (B, Lmax), clip b = wav[b, :lengths[b]]
        -> restored (B, Lmax), zero past a clip's end.  Every clip gets what its own restore_gsr(wav[b:b+1, :lengths[b]])
        computes (vfx_restore_gsr_varlen).  Any mix of lengths (round 6): the library runs the mel ResUNet once per padded frame
        count among the clips and the vocoder once over the whole batch."""
        wav, B, L, arr, out = self._varlen_args(wav, lengths, out, "restore_gsr_varlen")
        logmel = torch.empty((B, self.frames(L), N_MELS), device=self.device, dtype=torch.float32) if want_logmel else None
        _lib.check(self.lib.vfx_restore_gsr_varlen(self.h, _ptr(wav), B, L, arr, _ptr(out), _ptr(logmel),
                                                   int(bool(unify_energy)), self._stream()), "vfx_restore_gsr_varlen")
        return (out, logmel) if want_logmel else out

    def restore_ssr_varlen(self, wav, lengths, out=None):
        """ssr_unet / gsr_unet forward (sp = |STFT(wav)|, model(sp, wav)) for a batch of clips of UNEQUAL length: wav (B, Lmax),
        clip b = wav[b, :lengths[b]] -> (B, Lmax), zero past a clip's end; one `padded_frames` bucket per call."""
        wav, B, L, arr, out = self._varlen_args(wav, lengths, out, "restore_ssr_varlen")
        _lib.check(self.lib.vfx_restore_ssr_varlen(self.h, _ptr(wav), B, L, arr, _ptr(out), self._stream()), "vfx_restore_ssr_varlen")
        return out

    def _scored_args(self, target, target_lengths, B, L, name):
        """The target half of the two scored entries -> (target on the device or None, its lengths as the C int array or None)."""
        if target is not None:
            target = _dev_f32(target, self.device)
            target = target[None] if target.dim() == 1 else target
            if tuple(target.shape) != (B, L):
                raise ValueError("%s: target %s must have the shape of wav, (%d, %d)" % (name, tuple(target.shape), B, L))
        return target, self._lens_arg(target_lengths, B, name)

    def restore_gsr_varlen_scored(self, wav, lengths, target, target_lengths=None, unify_energy=False, want_logmel=False, out=None):
        """restore_gsr_varlen with the clips' targets (vfx_restore_gsr_varlen_scored): target (B, Lmax), clip b of it = its first
        target_lengths[b] samples (default: lengths) -> (restored (B, Lmax), scores (B, 4) float64 on the device[, logmel]).  The
        restored clips and the log-mel are those of restore_gsr_varlen bit for bit; the columns are models.HANDLER_METRIC_KEYS'
        order: mel-lsd, mel-sispec, mel-non-log-sispec, mel-ssim (eval_gsr_voicefixer.py:56-64), per clip over its own frames."""
        wav, B, L, arr, out = self._varlen_args(wav, lengths, out, "restore_gsr_varlen_scored")
        target, tarr = self._scored_args(target, target_lengths, B, L, "restore_gsr_varlen_scored")
        logmel = torch.empty((B, self.frames(L), N_MELS), device=self.device, dtype=torch.float32) if want_logmel else None
        scores = torch.empty((B, _lib.N_HANDLER_METRICS), device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_restore_gsr_varlen_scored(self.h, _ptr(wav), _ptr(target), B, L, arr, tarr, _ptr(out), _ptr(logmel),
                                                          _ptr(scores), int(bool(unify_energy)), self._stream()),
                   "vfx_restore_gsr_varlen_scored")
        return (out, scores, logmel) if want_logmel else (out, scores)

    def restore_ssr_varlen_scored(self, wav, lengths, target, target_lengths=None, out=None):
        """restore_ssr_varlen with the clips' targets (vfx_restore_ssr_varlen_scored; eval_ssr_unet.py:116-126) -> (restored (B, Lmax),
        scores (B, 4) float64 on the device, the same columns)."""
        wav, B, L, arr, out = self._varlen_args(wav, lengths, out, "restore_ssr_varlen_scored")
        target, tarr = self._scored_args(target, target_lengths, B, L, "restore_ssr_varlen_scored")
        scores = torch.empty((B, _lib.N_HANDLER_METRICS), device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_restore_ssr_varlen_scored(self.h, _ptr(wav), _ptr(target), B, L, arr, tarr, _ptr(out), _ptr(scores),
                                                          self._stream()), "vfx_restore_ssr_varlen_scored")
        return out, scores

    def spec_losses(self, est, target, lengths=None):
        """The three validation losses of waveform pairs, forward values only (vfx_spec_losses): est, target (B, L) or (L,), pair b =
        the first lengths[b] samples of row b (default: all L; 1024 < lengths[b] <= L) -> (B, 3) float64 on the device, the columns
        l1_wav, l1_sp, l1_log_sp (tools/pytorch/losses.py L1, L1_Sp, L1_Log_Sp) of each clip over its own samples and frames."""
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        if est.dim() == 1:
            est, target = est[None], target[None]
        if est.shape != target.shape or est.dim() != 2:
            raise ValueError("spec_losses: est %s and target %s must be equal (B, L) tensors" % (tuple(est.shape), tuple(target.shape)))
        B, L = est.shape
        out = torch.empty((B, _lib.N_SPEC_LOSSES), device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_spec_losses(self.h, _ptr(est), _ptr(target), B, L, self._lens_arg(lengths, B, "spec_losses"), _ptr(out),
                                            self._stream()), "vfx_spec_losses")
        return out

    def l1_rows(self, a, b, counts=None):
        """mean |a - b| over the first counts[r] elements (default: all) of every row of two equal (B, ...) float32 tensors, the rows
        flattened -> (B,) float64 on the device (vfx_l1_rows): the L1 of tensors that are not waveforms -- the log-mel case of
        losses.get_loss_function("l1") -- by the chunked float64 sums of spec_losses' column 0."""
        a, b = _dev_f32(a, self.device), _dev_f32(b, self.device)
        if a.shape != b.shape or a.dim() < 1:
            raise ValueError("l1_rows: a %s and b %s must have one shape" % (tuple(a.shape), tuple(b.shape)))
        B = a.shape[0] if a.dim() > 1 else 1
        a, b = a.reshape(B, -1), b.reshape(B, -1)
        out = torch.empty((B,), device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_l1_rows(self.h, _ptr(a), _ptr(b), B, a.shape[1], self._lens_arg(counts, B, "l1_rows"), _ptr(out),
                                        self._stream()), "vfx_l1_rows")
        return out

    def validate_gsr_varlen(self, wav, lengths, target, target_lengths=None, want_logmel=False):
        """val_l of VoiceFixer's validation_step per clip, without the vocoder (vfx_validate_gsr_varlen): wav, target (B, Lmax), clip b =
        wav[b, :lengths[b]], its target target[b, :target_lengths[b]] (default: lengths) -> val_l (B,) float64 on the device = the
        mean over the clip's own T_b x 128 values of |log-mel estimate - to_log(mel(target))| [, logmel (B, T, 128): bit for bit
        restore_gsr_varlen's].  Any mix of lengths; only the analysis module has to be loaded."""
        wav, _, B, L, lengths = _clip_rows(_dev_f32(wav, self.device), lengths, "validate_gsr_varlen")
        target, tarr = self._scored_args(target, target_lengths, B, L, "validate_gsr_varlen")
        logmel = torch.empty((B, self.frames(L), N_MELS), device=self.device, dtype=torch.float32) if want_logmel else None
        val_l = torch.empty((B,), device=self.device, dtype=torch.float64)
        _lib.check(self.lib.vfx_validate_gsr_varlen(self.h, _ptr(wav), _ptr(target), B, L, (ctypes.c_int * B)(*lengths), tarr, _ptr(logmel),
                                                    _ptr(val_l), self._stream()), "vfx_validate_gsr_varlen")
        return (val_l, logmel) if want_logmel else val_l

    def check_negative_input(self):
        """`to_log`'s assert alone (pytorch_util.py:158): reads and clears ONLY the negative-input bit -- a saturation bit a
        deferred vocoder check still has to see stays raised."""
        if self.take_flags(_lib.FLAG_NEGATIVE_INPUT) & _lib.FLAG_NEGATIVE_INPUT:
            raise AssertionError("to_log: input has negative values")

    def check_flags(self, rerun=None):
        """Reads and clears the handle's sticky device flags (one device sync, like `to_log`'s assert in the reference).
        A negative value reached a log10 -> AssertionError (pytorch_util.py:158), in every arithmetic mode.  16-bit vocoder
        (precision 2): an activation beyond the fp16 range was clamped -> the call is repeated on the split-bf16 twin
        (`rerun(twin_engine)`), or RuntimeError when no `rerun` is given.  Returns rerun's result, or None."""
        flags = self.take_flags()
        if flags & _lib.FLAG_NEGATIVE_INPUT:
            raise AssertionError("to_log: input has negative values")
        if flags & _lib.FLAG_F16_SATURATED:
            if rerun is None:
                raise RuntimeError("16-bit vocoder: an activation left the fp16 range (VFX_FLAG_F16_SATURATED); "
                                   "re-run with precision 1")
            import warnings
            warnings.warn("16-bit vocoder: an activation left the fp16 range; this call is re-run with split-bf16 operands")
            try:
                twin = self.strict_twin()
            except RuntimeError as e:      # a second copy of the weights + its arena on the same GPU, mid-run
                raise RuntimeError("16-bit vocoder: the split-bf16 twin this call must be re-run on could not be created "
                                   "(%s); call Engine.strict_twin() once at start-up to reserve it, or use precision 1" % e)
            return rerun(twin)
        return None

    def restore_gsr_checked(self, wav, unify_energy=False, out=None):
        """restore_gsr + check_flags: never silently wrong in the 16-bit mode, whoever the caller is (models, dist, bench)."""
        res = self.restore_gsr(wav, unify_energy=unify_energy, out=out)
        again = self.check_flags(lambda e: e.restore_gsr(wav, unify_energy=unify_energy, out=out))
        return res if again is None else again

    def restore_gsr_varlen_checked(self, wav, lengths, unify_energy=False, out=None):
        """restore_gsr_varlen + check_flags (cf. restore_gsr_checked)."""
        res = self.restore_gsr_varlen(wav, lengths, unify_energy=unify_energy, out=out)
        again = self.check_flags(lambda e: e.restore_gsr_varlen(wav, lengths, unify_energy=unify_energy, out=out))
        return res if again is None else again

    def restore_gsr_varlen_scored_checked(self, wav, lengths, target, target_lengths=None, unify_energy=False, out=None):
        """restore_gsr_varlen_scored + check_flags: a batch the 16-bit vocoder clamped is restored AND scored again on the strict twin."""
        res = self.restore_gsr_varlen_scored(wav, lengths, target, target_lengths, unify_energy=unify_energy, out=out)
        again = self.check_flags(lambda e: e.restore_gsr_varlen_scored(wav, lengths, target, target_lengths, unify_energy=unify_energy,
                                                                       out=out))
        return res if again is None else again

    def vocoder_checked(self, mel_linear):
        res = self.vocoder(mel_linear)
        again = self.check_flags(lambda e: e.vocoder(mel_linear))
        return res if again is None else again

    def profile_begin(self):
        _lib.check(self.lib.vfx_profile_begin(self.h), "vfx_profile_begin")

    def profile_end(self):
        """-> (launches, total_ms, total_flops) of the tap-convolution launches since profile_begin."""
        n, ms, fl = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
        _lib.check(self.lib.vfx_profile_end(self.h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)), "vfx_profile_end")
        return n.value, ms.value, fl.value

    # ------------------------------------------------------------------ kernel-level ops (tests: libvfx_test.so, include/vfx_test.h)
    def op_conv(self, x, weight, scale=None, shift=None, act=0, slope=0.0, bias=None, residual=None, dil_w=1,
                reflect_w=False):
        """x (B,H,W,Cin) channels-last; weight (Cout,Cin,kh,kw) torch layout (host)."""
        x = _dev_f32(x, self.device)
        B, H, W, Cin = x.shape
        w = _host(weight)
        Cout, _, kh, kw = w.shape
        y = torch.empty((B, H, W, Cout), device=self.device, dtype=torch.float32)
        scale, shift, bias = _host(scale), _host(shift), _host(bias)
        res = None if residual is None else _dev_f32(residual, self.device)
        _lib.check(_lib.load_test().vfx_op_conv(self.h, _ptr(x), B, H, W, Cin, _hptr(w), Cout, kh, kw, dil_w, int(reflect_w),
                                                _hptr(scale), _hptr(shift), act, float(slope), _hptr(bias), _ptr(res), _ptr(y),
                                                self._stream()), "vfx_op_conv")
        return y

    def op_resblock(self, x, w1, b1, w2, b2, dil, slope=0.01, fused=True):
        """One ResStack layer on x (B, T, C) channels-last; w1 / w2 (C, C, 3), b1 / b2 (C) torch layout (host)."""
        x = _dev_f32(x, self.device)
        B, T, C = x.shape
        layer = [_host(a) for a in (w1, b1, w2, b2)]
        y = torch.empty_like(x)
        _lib.check(_lib.load_test().vfx_op_resblock(self.h, _ptr(x), B, T, C, *[_hptr(a) for a in layer], int(dil), float(slope),
                                                    int(bool(fused)), _ptr(y), self._stream()), "vfx_op_resblock")
        return y

    def op_resblock_pair(self, x, layer_a, dil_a, layer_b, dil_b, slope=0.01):
        """Two consecutive ResStack layers as one launch (16-bit mode, C = 64); layer_* = (w1, b1, w2, b2) in torch layout."""
        x = _dev_f32(x, self.device)
        B, T, C = x.shape
        la, lb = [_host(a) for a in layer_a], [_host(a) for a in layer_b]
        y = torch.empty_like(x)
        _lib.check(_lib.load_test().vfx_op_resblock_pair(self.h, _ptr(x), B, T, C, *[_hptr(a) for a in la[:4]], int(dil_a),
                                                         *[_hptr(a) for a in lb[:4]], int(dil_b), float(slope), _ptr(y),
                                                         self._stream()), "vfx_op_resblock_pair")
        return y

    def op_block2d(self, x, w1, sc1, sh1, w2, sc2, sh2, slope=0.01):
        """One fused ConvBlockRes (identity shortcut) on x (B, H, W, C) channels-last; w1 / w2 (C, C, 3, 3) and the folded
        BatchNorm affines (C) in torch layout on the host."""
        x = _dev_f32(x, self.device)
        B, H, W, C = x.shape
        block = [_host(a) for a in (w1, sc1, sh1, w2, sc2, sh2)]
        y = torch.empty_like(x)
        _lib.check(_lib.load_test().vfx_op_block2d(self.h, _ptr(x), B, H, W, C, *[_hptr(a) for a in block], float(slope), _ptr(y),
                                                   self._stream()), "vfx_op_block2d")
        return y

    def op_conv_transpose(self, x, weight, stride, prune_w=False, scale=None, shift=None, act=0, slope=0.0, bias=None):
        x = _dev_f32(x, self.device)
        B, H, W, Cin = x.shape
        w = _host(weight)
        _, Cout, kh, kw = w.shape
        if kh == 3:
            shape = (B, 2 * H, 2 * W if prune_w else 2 * W + 1, Cout)
        else:
            shape = (B, 1, W * stride, Cout)
        y = torch.empty(shape, device=self.device, dtype=torch.float32)
        scale, shift, bias = _host(scale), _host(shift), _host(bias)
        _lib.check(_lib.load_test().vfx_op_conv_transpose(self.h, _ptr(x), B, H, W, Cin, _hptr(w), Cout, kh, kw, stride, int(prune_w),
                                                          _hptr(scale), _hptr(shift), act, float(slope), _hptr(bias), _ptr(y),
                                                          self._stream()), "vfx_op_conv_transpose")
        return y

    # the vocoder's launches as its plan builds them (include/vfx_test.h: vfx_op_voc_*)
    OP_STORED = 0x100   # VFX_OP_STORED (include/vfx_test.h)

    def stored_tensor(self, shape):
        """A device buffer for an ACTIVATED tensor of `shape` in the form the launches of this handle store it (`stored=True` of
        op_voc_upsample / op_voc_conv1d): fp16 in the 16-bit mode; otherwise four bytes per element -- fp32 values in the fp32 mode,
        the packed bf16 pairs of the split-bf16 mode, which are no fp32 values.  Starts as NaN patterns."""
        t = torch.empty(shape, device=self.device, dtype=torch.float16 if self.precision == 2 else torch.float32)
        t.view(torch.uint8).fill_(0xff)
        return t

    def _stored_arg(self, t, name):
        want = torch.float16 if self.precision == 2 else torch.float32
        if not (isinstance(t, torch.Tensor) and t.dtype == want and t.is_cuda and t.is_contiguous()):
            raise ValueError("%s: a stored tensor is a contiguous %s device tensor (Engine.stored_tensor)" % (name, want))
        return t

    def op_voc_upsample(self, x, weight, bias, stride, up_slope=0.2, src_act=True, want_raw=False, act_slope=None, lens=None,
                        stored=False):
        """One upsampler on x (B, T, Cin): -> (y raw or None, ya activated or None, ran_on_k_up16).  act_slope None: no activated
        output; 1.0: the fp16 trunk of the 16-bit mode.  y starts as NaN, so do unwritten elements of ya.  stored: the activated
        tensors -- x where src_act, ya -- cross the call as the launches store them (stored_tensor), byte for byte."""
        x = self._stored_arg(x, "op_voc_upsample") if stored and src_act else _dev_f32(x, self.device)
        B, T, Cin = x.shape
        w, b = _host(weight), _host(bias)
        Cout = w.shape[1]
        shape = (B, T * stride, Cout)
        y = torch.full(shape, float("nan"), device=self.device) if want_raw else None
        ya = None if act_slope is None else (self.stored_tensor(shape) if stored else torch.empty(shape, device=self.device))
        ln = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
        up16 = ctypes.c_int(-1)
        st = self.OP_STORED if stored else 0
        _lib.check(_lib.load_test().vfx_op_voc_upsample(
            self.h, _ptr(x), B, T, Cin, _hptr(w), _hptr(b), int(stride), float(up_slope), (1 | st) if src_act else 0, int(bool(want_raw)),
            (1 | st) if act_slope is not None else 0, float(act_slope if act_slope is not None else 1.0), _hptr(ln), _ptr(y), _ptr(ya),
            ctypes.byref(up16), self._stream()), "vfx_op_voc_upsample")
        return y, ya, bool(up16.value)

    def op_voc_conv1d(self, x, weight, bias, dil=1, reflect=False, src_act=False, act=0, slope=1.0, residual=None, residual_act=False,
                      want_raw=True, next_act=0, next_slope=1.0, lens=None, stored=False):
        """Conv1d of the vocoder plan on x (B, T, Cin): -> (y raw or None, ya activated or None); both start as NaN.  stored: the
        activated tensors -- x where src_act, the residual where residual_act (fp16), ya -- cross the call as the launches store
        them (stored_tensor), byte for byte.  self.last_conv_w64: the plan that ran put the launch on k_conv_w64."""
        x = self._stored_arg(x, "op_voc_conv1d") if stored and src_act else _dev_f32(x, self.device)
        B, T, Cin = x.shape
        w, b = _host(weight), _host(bias)
        Cout, _, K = w.shape
        y = torch.full((B, T, Cout), float("nan"), device=self.device) if want_raw else None
        ya = None if not next_act else (self.stored_tensor((B, T, Cout)) if stored else torch.empty((B, T, Cout), device=self.device))
        if residual is None:
            res = None
        elif stored and residual_act:
            res = residual
            if not (res.dtype == torch.float16 and res.is_cuda and res.is_contiguous()):
                raise ValueError("op_voc_conv1d: a stored activated residual is a contiguous fp16 device tensor")
        else:
            res = _dev_f32(residual, self.device)
        ln = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
        st = self.OP_STORED if stored else 0
        w64 = ctypes.c_int(-1)
        _lib.check(_lib.load_test().vfx_op_voc_conv1d(
            self.h, _ptr(x), B, T, Cin, _hptr(w), _hptr(b), Cout, K, int(dil), int(bool(reflect)), (1 | st) if src_act else 0, int(act),
            float(slope), _ptr(res), (1 | st) if residual_act else 0, int(bool(want_raw)), int(next_act) | (st if next_act else 0),
            float(next_slope), _hptr(ln), _ptr(y), _ptr(ya), ctypes.byref(w64), self._stream()), "vfx_op_voc_conv1d")
        self.last_conv_w64 = bool(w64.value)
        return y, ya

    def op_voc_final(self, x, weight, bias, slope=0.2, x_f16=False, lens=None, want_peak=False):
        """The vocoder tail on x (B, T, C): -> wav (B, T), NaN where nothing was written.  want_peak: -> (wav, peak (B,)), the per-clip
        max |wav| the tail hands the peak normalisation (starts as NaN)."""
        x = _dev_f32(x, self.device)
        B, T, C = x.shape
        w = _host(weight)
        wav = torch.full((B, T), float("nan"), device=self.device)
        peak = torch.full((B,), float("nan"), device=self.device) if want_peak else None
        ln = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
        _lib.check(_lib.load_test().vfx_op_voc_final(
            self.h, _ptr(x), B, T, C, _hptr(w), float(bias), float(slope), int(bool(x_f16)), _hptr(ln), _ptr(wav), _ptr(peak),
            self._stream()), "vfx_op_voc_final")
        return (wav, peak) if want_peak else wav

    RESBLOCK_INFO = ("rw", "r128", "asrc", "fold", "tile_m", "TWo", "TH", "tiles_h", "tiles_w", "x16", "W1", "patch_rows")

    def op_voc_resblock(self, x, layer, dil, layer2=None, dil2=0, slope=0.01, act_slope=0.2, want_raw=True, want_act=False, lens=None,
                        lens_mul=1):
        """One fused ResStack launch of the vocoder plan on x (B, T, C): layer = (w1, b1, w2, b2) in torch layout, layer2 / dil2 the
        second layer of a pair.  -> (y raw or None, ya activated or None, info): both widened from the stored form, NaN where the
        launch stored nothing; info = what plan_resblock chose (RESBLOCK_INFO).  Raises where the plan refuses the combination."""
        x = _dev_f32(x, self.device)
        B, T, C = x.shape
        la = [_host(a) for a in layer]
        lb = [_host(a) for a in layer2] if layer2 is not None else [None] * 4
        y = torch.full_like(x, float("nan")) if want_raw else None
        ya = torch.full_like(x, float("nan")) if want_act else None
        ln = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
        if ln is not None and ln.shape != (B,):
            raise ValueError("op_voc_resblock: %d lengths for %d clips" % (ln.size, B))
        info = (ctypes.c_int * len(self.RESBLOCK_INFO))()
        _lib.check(_lib.load_test().vfx_op_voc_resblock(
            self.h, _ptr(x), B, T, C, *[_hptr(a) for a in la], int(dil), *[_hptr(a) for a in lb], int(dil2 if layer2 is not None else 0),
            float(slope), float(act_slope), int(bool(want_raw)), int(bool(want_act)), _hptr(ln), int(lens_mul), _ptr(y), _ptr(ya), info,
            self._stream()), "vfx_op_voc_resblock")
        return y, ya, dict(zip(self.RESBLOCK_INFO, info))

    def op_voc_resblock_at(self, x, xa, layer, dil, layer2=None, dil2=0, slope=0.01, act_slope=0.2, last_stage=False, want_raw=True,
                           want_act=False):
        """op_voc_resblock at a stated place of the plan: last_stage -- the stack in front of the tail -- and xa, the activated fp16
        trunk of a wide layer as the launch in front of it stored it (an fp16 device tensor; None for the other widths); x is None
        where xa is the trunk's only form.  -> (y, ya, info) as op_voc_resblock."""
        x = None if x is None else _dev_f32(x, self.device)
        if xa is not None and not (xa.dtype == torch.float16 and xa.is_cuda and xa.is_contiguous()):
            raise ValueError("op_voc_resblock_at: xa is a contiguous fp16 device tensor")
        B, T, C = (x if x is not None else xa).shape
        la = [_host(a) for a in layer]
        lb = [_host(a) for a in layer2] if layer2 is not None else [None] * 4
        y = torch.full((B, T, C), float("nan"), device=self.device) if want_raw else None
        ya = torch.full((B, T, C), float("nan"), device=self.device) if want_act else None
        info = (ctypes.c_int * len(self.RESBLOCK_INFO))()
        _lib.check(_lib.load_test().vfx_op_voc_resblock_at(
            self.h, _ptr(x), _ptr(xa), B, T, C, *[_hptr(a) for a in la], int(dil), *[_hptr(a) for a in lb],
            int(dil2 if layer2 is not None else 0), float(slope), float(act_slope), int(bool(last_stage)), int(bool(want_raw)),
            int(bool(want_act)), _ptr(y), _ptr(ya), info, self._stream()), "vfx_op_voc_resblock_at")
        return y, ya, dict(zip(self.RESBLOCK_INFO, info))

    VOC_STACK_KINDS = ("two_launches", "fused", "fused_wide")

    def plan_voc_stack(self, C, last_stage=False, dil=1, dil2=0):
        """How this handle's vocoder plan runs the ResStack of C channels (no launch) -> (kind, one of VOC_STACK_KINDS; the trunk
        between its launches is fp16; the layers of dilation dil and dil2 run as one launch)."""
        out = (ctypes.c_int * 3)()
        _lib.check(_lib.load_test().vfx_plan_voc_stack(self.h, int(C), int(bool(last_stage)), int(dil), int(dil2), out), "vfx_plan_voc_stack")
        return self.VOC_STACK_KINDS[out[0]], bool(out[1]), bool(out[2])

    # the STFT / ISTFT front end and the glue launches of a restore call (include/vfx_test.h); every output starts as NaN
    @staticmethod
    def _lens_arg(lens, B, name):
        if lens is None:
            return None
        lens = [int(v) for v in lens]
        if len(lens) != B:
            raise ValueError("%s: %d lengths for %d clips" % (name, len(lens), B))
        return (ctypes.c_int * B)(*lens)

    def op_stft(self, wav, T=None, lens=None, eps=1e-8, log10_mel=False, want=("mel", "sp", "cos", "sin")):
        """launch_stft_mel on wav (B, L): -> dict of the outputs named in `want`, mel (B, T, 128), sp / cos / sin (B, T, 1025).  T: the row
        stride of the outputs (default frames(L)); lens: samples per clip, as the varlen callers pass them."""
        wav = _dev_f32(wav, self.device)
        B, L = wav.shape
        T = self.frames(L) if T is None else int(T)
        out = {k: torch.full((B, T, N_MELS if k == "mel" else N_BINS), float("nan"), device=self.device) for k in want}
        _lib.check(_lib.load_test().vfx_op_stft(
            self.h, _ptr(wav), B, L, T, self._lens_arg(lens, B, "op_stft"), float(eps), int(bool(log10_mel)), _ptr(out.get("mel")),
            _ptr(out.get("sp")), _ptr(out.get("cos")), _ptr(out.get("sin")), self._stream()), "vfx_op_stft")
        return out

    def op_istft(self, re, im, length, lens=None):
        """launch_istft on re, im (B, T, 1025): -> wav (B, length); lens: samples per clip."""
        re, im = _dev_f32(re, self.device), _dev_f32(im, self.device)
        B, T, _ = re.shape
        wav = torch.full((B, int(length)), float("nan"), device=self.device)
        _lib.check(_lib.load_test().vfx_op_istft(self.h, _ptr(re), _ptr(im), B, T, int(length), self._lens_arg(lens, B, "op_istft"),
                                                 _ptr(wav), self._stream()), "vfx_op_istft")
        return wav

    @staticmethod
    def plan_stft_frames_per_group(frames):
        """Host-only: the frames one wave of k_stft_mel walks in a launch of `frames` = B * T frames.  Needs no GPU."""
        return int(_lib.load_test().vfx_plan_stft_frames_per_group(int(frames)))

    @staticmethod
    def plan_istft_grid(B, T, L):
        """Host-only: (IH, workgroups per clip) of the k_istft launch for (B, T, L).  Needs no GPU."""
        out = (ctypes.c_int * 2)()
        _lib.check(_lib.load_test().vfx_plan_istft_grid(int(B), int(T), int(L), out), "vfx_plan_istft_grid")
        return out[0], out[1]

    def op_from_log(self, logmel, mel_in=None, unify=False, lens_t=None):
        """launch_from_log on logmel (B, T, 128) (and mel_in, the target of unify): -> mel_out (B, T, 128)."""
        logmel = _dev_f32(logmel, self.device)
        mel_in = None if mel_in is None else _dev_f32(mel_in, self.device)
        B, T, _ = logmel.shape
        out = torch.full_like(logmel, float("nan"))
        _lib.check(_lib.load_test().vfx_op_from_log(self.h, _ptr(logmel), _ptr(mel_in), B, T, int(bool(unify)),
                                                    self._lens_arg(lens_t, B, "op_from_log"), _ptr(out), self._stream()),
                   "vfx_op_from_log")
        return out

    def op_voc_prep(self, mel, Tp, lens_t=None):
        """launch_voc_prep on mel (B, T, 128) linear: -> cond (B, Tp, 128)."""
        mel = _dev_f32(mel, self.device)
        B, T, _ = mel.shape
        cond = torch.full((B, int(Tp), N_MELS), float("nan"), device=self.device)
        _lib.check(_lib.load_test().vfx_op_voc_prep(self.h, _ptr(mel), B, T, int(Tp), self._lens_arg(lens_t, B, "op_voc_prep"),
                                                    _ptr(cond), self._stream()), "vfx_op_voc_prep")
        return cond

    def op_peak_trim(self, wav_long, L, peak, lens_l=None, lens_tp=None):
        """launch_peak_trim (launch_peak_trim_varlen with lens_l, lens_tp) on wav_long (B, Llong) and the per-clip peaks (host): ->
        out (B, L).  The flag a division raises stays in the handle's flag word for take_flags()."""
        wav_long = _dev_f32(wav_long, self.device)
        B, Llong = wav_long.shape
        pk = _host(peak)
        if pk.shape != (B,):
            raise ValueError("op_peak_trim: %s peaks for %d clips" % (pk.shape, B))
        out = torch.full((B, int(L)), float("nan"), device=self.device)
        _lib.check(_lib.load_test().vfx_op_peak_trim(
            self.h, _ptr(wav_long), B, Llong, int(L), _hptr(pk), self._lens_arg(lens_l, B, "op_peak_trim"),
            self._lens_arg(lens_tp, B, "op_peak_trim"), _ptr(out), self._stream()), "vfx_op_peak_trim")
        return out

    # the ResUNet plans' launches, one piece at a time, built by the plan's own builder (include/vfx_test.h: vfx_op_unet_piece)
    UNET_LAUNCH_FAMILIES = ("small", "k_conv", "k_conv_phased", "k_resblock", "k_resblock_in1", "k_resblock_two_src", "k_block2d32")

    @staticmethod
    def _unet_launches(buf, n):
        keys = ("family", "ksplit", "out_act", "bias", "nseg", "cout")
        rows = [dict(zip(keys, buf[6 * i:6 * i + 6])) for i in range(n)]
        for r in rows:
            r["family"] = Engine.UNET_LAUNCH_FAMILIES[r["family"]]
        return rows

    @staticmethod
    def _unet_piece_out_shapes(piece, in_shapes, arg):
        B, H, W = in_shapes[0][:3]
        if piece == "entry":
            return [(B, H, W, 32)]
        if piece.endswith(".up"):
            cout = {1: 384, 2: 384, 3: 256, 4: 128, 5: 64, 6: 32}[int(piece[3])]
            return [(B, 2 * H, 2 * W if arg else 2 * W + 1, cout)]
        if piece == "pool":
            return [(B, H // 2, W // 2, in_shapes[0][3])]
        if piece in ("prep_logmel", "prep_spec"):
            return [(B, (H + 63) // 64 * 64, W - 1)]
        if piece == "final":
            return [tuple(in_shapes[1])] * (2 if arg else 1)
        if piece.startswith("dec") and piece.endswith(".1"):
            return [tuple(in_shapes[0])]
        cout = {"enc2.1": 64, "enc3.1": 128, "enc4.1": 256, "enc5.1": 384}.get(piece, in_shapes[0][3])
        return [(B, H, W, cout)]

    def op_unet_piece(self, piece, inputs, arg=0, short_clip=0, lens=None, model=MODEL_UNET_MEL):
        """One piece of the ResUNet plan of `model` on device tensors -> (outputs, h, launches).  inputs: the piece's channels-last
        tensors (include/vfx_test.h); outputs start as NaN.  h: the tensor between the two launches of a block's two-launch form,
        widened to fp32, as ("act" | "raw", tensor), or None for a single launch.  launches: as plan_unet_piece.  For "final",
        inputs[0] is the trunk's (B, Tpad, W, 32) output and the frame count is inputs[1]'s."""
        xs = [_dev_f32(x, self.device) for x in inputs]
        shapes = [tuple(x.shape) for x in xs]
        outs = [torch.full(sh, float("nan"), device=self.device) for sh in self._unet_piece_out_shapes(piece, shapes, arg)]
        if piece == "final":
            B, H, W = shapes[1][0], shapes[1][1], shapes[0][2]
        else:
            B, H, W = shapes[0][:3]
        hbuf = torch.full(outs[0].shape, float("nan"), device=self.device)
        ln = None if lens is None else np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
        pin = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        pout = (ctypes.c_void_p * len(outs))(*[y.data_ptr() for y in outs])
        nin = (ctypes.c_int64 * len(xs))(*[x.numel() for x in xs])
        nout = (ctypes.c_int64 * len(outs))(*[y.numel() for y in outs])
        form, n, buf = ctypes.c_int(-1), ctypes.c_int(0), (ctypes.c_int * 48)()
        _lib.check(_lib.load_test().vfx_op_unet_piece(
            self.h, int(model), piece.encode(), B, H, W, int(arg), int(short_clip), _hptr(ln), pin, nin, len(xs), pout, nout, len(outs),
            _ptr(hbuf), hbuf.numel(), ctypes.byref(form), buf, 48, ctypes.byref(n), self._stream()), "vfx_op_unet_piece")
        h = None if form.value < 0 else (("raw", "act")[form.value], hbuf)
        return outs, h, self._unet_launches(buf, min(n.value, 8))

    @staticmethod
    def plan_unet_piece(piece, B, H, W, arg=0, short_clip=0, precision=1, tuning=0):
        """Host-only: the launches the ResUNet plan builds for `piece` over (B, H, W): a list of dicts with family (one of
        UNET_LAUNCH_FAMILIES), ksplit (1 = no split-K), out_act, bias, nseg, cout.  Needs no GPU."""
        n, buf = ctypes.c_int(0), (ctypes.c_int * 48)()
        _lib.check(_lib.load_test().vfx_plan_unet_piece(piece.encode(), B, H, W, int(arg), int(short_clip), int(precision), int(tuning),
                                                        buf, 48, ctypes.byref(n)), "vfx_plan_unet_piece")
        return Engine._unet_launches(buf, min(n.value, 8))

    @staticmethod
    def plan_unet(model, B, T, precision=1, tuning=0):
        """Host-only: the launches of the WHOLE plan of resunet_mel (MODEL_UNET_MEL) / resunet_spec (MODEL_UNET_SPEC) for B clips of T
        frames, as plan_unet_piece reports a piece's: the small kernels, then the fused blocks, then the convolutions, each group
        in launch order.  Needs no GPU."""
        cap = 6 * 512
        n, buf = ctypes.c_int(0), (ctypes.c_int * cap)()
        _lib.check(_lib.load_test().vfx_plan_unet(int(model), int(B), int(T), int(precision), int(tuning), buf, cap, ctypes.byref(n)),
                   "vfx_plan_unet")
        if n.value * 6 > cap:
            raise RuntimeError("plan_unet: %d launches" % n.value)
        return Engine._unet_launches(buf, n.value)

    # the bi_gru / dnn plans' launches, one at a time, built by the plan's own builder (include/vfx_test.h: vfx_op_analysis_piece)
    ANALYSIS_PIECE_WIDTHS = {"lin1": 256, "proj0": 1536, "gru0": 512, "proj1": 1536, "gru1": 512, "lin4": 256, "lin6": 128,
                             "fc0": 256, "fc1": 512, "fc2": 1024, "fc3": 512, "fc4": 256, "fc5": 128}

    def op_analysis_piece(self, model, piece, inputs, lens=None):
        """One launch of the analysis plan of `model` (MODEL_GRU_MEL: lin1, proj0, gru0, proj1, gru1, lin4, lin6; MODEL_DNN_MEL: fc0 ..
        fc5) on device tensors (B, T, C) -> its output (B, T, C'), which starts as NaN.  inputs: one tensor, for lin6 / fc5 two (the
        second the linear mel).  lens: frames per clip, as analysis_mel's `frames`."""
        xs = [_dev_f32(x, self.device) for x in inputs]
        B, T = xs[0].shape[:2]
        out = torch.full((B, T, self.ANALYSIS_PIECE_WIDTHS[piece]), float("nan"), device=self.device)
        pin = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        nin = (ctypes.c_int64 * len(xs))(*[x.numel() for x in xs])
        _lib.check(_lib.load_test().vfx_op_analysis_piece(
            self.h, int(model), piece.encode(), B, T, self._lens_arg(lens, B, "op_analysis_piece"), pin, nin, len(xs), _ptr(out),
            out.numel(), self._stream()), "vfx_op_analysis_piece")
        return out

    def op_ssim(self, est, target, rows=None):
        """The SSIM kernels of audio_metrics alone: (B, T, F) images, image b = its first rows[b] rows -> (B,) float64."""
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        B, T, F = est.shape
        rows = _clip_rows(est[:, :, 0], rows, "op_ssim")[4]
        out = torch.empty(B, device=self.device, dtype=torch.float64)
        _lib.check(_lib.load_test().vfx_op_ssim(self.h, _ptr(est), _ptr(target), B, T, F, (ctypes.c_int * B)(*rows), _ptr(out),
                                                self._stream()), "vfx_op_ssim")
        return out

    def op_handler_metrics(self, logmel, den, target_mel, frames=None):
        """The scoring launches of restore_gsr_varlen_scored alone (vfx_op_handler_metrics): (B, T, 128) images -- the log10 estimate, what
        the vocoder receives, the target's linear mel --, clip b = their first frames[b] rows -> (B, 4) float64."""
        logmel, den, target_mel = (_dev_f32(t, self.device) for t in (logmel, den, target_mel))
        B, T, _ = logmel.shape
        frames = _clip_rows(logmel[:, :, 0], frames, "op_handler_metrics")[4]
        out = torch.full((B, _lib.N_HANDLER_METRICS), float("nan"), device=self.device, dtype=torch.float64)
        _lib.check(_lib.load_test().vfx_op_handler_metrics(self.h, _ptr(logmel), _ptr(den), _ptr(target_mel), B, T,
                                                           (ctypes.c_int * B)(*frames), _ptr(out), self._stream()), "vfx_op_handler_metrics")
        return out

    def op_mel_metrics(self, est_mel, target_mel, frames=None):
        """The scoring launches of restore_ssr_varlen_scored alone (vfx_op_mel_metrics): the same four scores of (est_mel, target_mel)."""
        est_mel, target_mel = _dev_f32(est_mel, self.device), _dev_f32(target_mel, self.device)
        B, T, _ = est_mel.shape
        frames = _clip_rows(est_mel[:, :, 0], frames, "op_mel_metrics")[4]
        out = torch.full((B, _lib.N_HANDLER_METRICS), float("nan"), device=self.device, dtype=torch.float64)
        _lib.check(_lib.load_test().vfx_op_mel_metrics(self.h, _ptr(est_mel), _ptr(target_mel), B, T, (ctypes.c_int * B)(*frames),
                                                       _ptr(out), self._stream()), "vfx_op_mel_metrics")
        return out

    def op_sisdr(self, est, target, lengths=None):
        """The SI-SDR kernels of audio_metrics alone: (B, L), clip b = its first lengths[b] samples -> (B,) float64 dB."""
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        est, _, B, L, lengths = _clip_rows(est, lengths, "op_sisdr")
        out = torch.empty(B, device=self.device, dtype=torch.float64)
        _lib.check(_lib.load_test().vfx_op_sisdr(self.h, _ptr(est), _ptr(target), B, L, (ctypes.c_int * B)(*lengths), _ptr(out),
                                                 self._stream()), "vfx_op_sisdr")
        return out

    def op_score_spectrogram(self, wav, lengths=None, rate=16000):
        """The two images audio_metrics scores, of one signal (vfx_op_score_spectrogram): wav (B, L) or (L,), clip b = its first
        lengths[b] samples -> (sp (B, T, 372), mel (B, T, 80)) at 16 kHz, (B, T, 1025) and (B, T, 128) at 44.1 kHz; T = the frames of
        the longest clip (1 + (n - 1) // 160, n // 441 + 1), rows at or past a clip's own frames are zeros."""
        wav = _dev_f32(wav, self.device)
        wav, _, B, L, lengths = _clip_rows(wav, lengths, "op_score_spectrogram")
        rate = int(rate)
        hop, F, M = (160, 372, 80) if rate == 16000 else (self.cfg.hop, self.cfg.n_fft // 2 + 1, self.cfg.n_mels)
        T = max([1 + (n - 1) // 160 if rate == 16000 else n // hop + 1 for n in lengths] + [1])
        sp = torch.empty((B, T, F), device=self.device, dtype=torch.float32)
        mel = torch.empty((B, T, M), device=self.device, dtype=torch.float32)
        self._score_tables(rate)
        _lib.check(_lib.load_test().vfx_op_score_spectrogram(self.h, _ptr(wav), B, L, (ctypes.c_int * max(B, 1))(*lengths), rate,
                                                             _ptr(sp), _ptr(mel), self._stream()), "vfx_op_score_spectrogram")
        return sp, mel

    STOI_STAGES = ("resampled", "mask", "powers", "tob")

    def op_stoi_stage(self, stage, est, target, lengths=None, fs=44100):
        """One intermediate of `stoi` for the whole batch (vfx_op_stoi_stage), as float64 / int32 tensors on the device; N = the
        longest clip's samples at 10 kHz, Fm = max(1, its frames); entries past a clip's own extent are zero:
          "resampled" -> (est and target at 10 kHz (B, 2, N), each clip's samples at 10 kHz (B,))
          "mask"      -> (the target's frame energies in dB (B, Fm), kept counts (B,), the keep mask (B, Fm))
          "powers"    -> (band powers of est and target per STFT frame (B, 2, Fm, 15), kept counts (B,)): frames m < kept - 1
          "tob"       -> (their square roots, kept counts)"""
        k = self.STOI_STAGES.index(stage)
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        if est.dim() == 1:
            est, target = est[None], target[None]
        est, _, B, L, lengths = _clip_rows(est, lengths, "op_stoi_stage")
        up, down, taps, ntaps = self.stoi_taps(fs)
        N = max(1, -(-max(lengths) * up // down))
        Fm = max(1, -(-(N - 256) // 128))
        shape = ((B, 2, N), (B, Fm), (B, 2, Fm, 15), (B, 2, Fm, 15))[k]
        out = torch.zeros(shape, device=self.device, dtype=torch.float64)
        iout = torch.zeros(B * (1 + Fm) if k == 1 else B, device=self.device, dtype=torch.int32)
        _lib.check(_lib.load_test().vfx_op_stoi_stage(self.h, _ptr(est), _ptr(target), B, L, (ctypes.c_int * B)(*lengths), up, down,
                                                      _ptr(taps) if taps is not None else None, ntaps, k, _ptr(out), out.numel(),
                                                      _ptr(iout), iout.numel(), self._stream()), "vfx_op_stoi_stage")
        if k == 1:
            return out, iout[:B], iout[B:].view(B, Fm)
        return out, iout

    BSSEVAL_STAGES = ("lags", "filter", "energies", "projection")

    def op_bsseval_stage(self, stage, est, target, lengths=None, flen=512):
        """One intermediate of `bsseval` for the whole batch (vfx_op_bsseval_stage), a float64 tensor on the device:
          "lags"       -> (B, 2, flen): a and d
          "filter"     -> (B, flen): c
          "energies"   -> (B, 5): sum r^2, (e - r)^2, (P - r)^2, P^2, (e - P)^2
          "projection" -> (B, L + flen - 1): P, zeros past a clip's own lengths[b] + flen - 1"""
        k = self.BSSEVAL_STAGES.index(stage)
        est, target = _dev_f32(est, self.device), _dev_f32(target, self.device)
        if est.dim() == 1:
            est, target = est[None], target[None]
        est, _, B, L, lengths = _clip_rows(est, lengths, "op_bsseval_stage")
        flen = int(flen)
        shape = ((B, 2, flen), (B, flen), (B, 5), (B, L + flen - 1))[k]
        out = torch.zeros(shape, device=self.device, dtype=torch.float64)
        _lib.check(_lib.load_test().vfx_op_bsseval_stage(self.h, _ptr(est), _ptr(target), B, L, (ctypes.c_int * B)(*lengths), flen, k,
                                                         _ptr(out), out.numel(), self._stream()), "vfx_op_bsseval_stage")
        return out
