"""Silence and activity: the peak-threshold functions of the reference's data preparation (tools/others/audio_op.py:71-150), with the
reference's names, signatures and defaults for one NumPy clip, and their list forms on the device (Engine.trim_bounds /
has_long_empty / active_frames, csrc/activity.hip):

* ``trim_tail_empty`` / ``trim_head_empty`` / ``trim_empty(wave, threshold=500, sample_rate=44100, frame_length=0.02)``
* ``has_long_empty(wave, length=3, sample_rate=44100)`` (its 400 is the keyword ``threshold`` here)
* ``get_all_active_segment_index(wave, threshold=500, sample_rate=44100, frame_length=0.02, frame_shift=0.01)``
* ``is_valid_signal(wave, threshold=1000)`` and ``max_mag_unify(ref, est)``

Everything is decided by window peaks max |x[i]| over windows of the clip, and every host form here is the CLOSED form over those
peaks that the kernels evaluate (``tail_stop``, ``head_start``: a last / first active window by index), not the reference's walk;
tests/test_activity_host.py holds them to a transcription of the walks.  The quirks of the walks are kept: the tail drops one further
segment once it has dropped any and can leave an EMPTY clip, the head keeps one quiet segment, a clip of exactly one segment passes the
tail and fails the head.  The trims return None exactly where the reference does.

A float clip is compared with ``x.dtype.type(threshold)``: what NumPy >= 2 does with a Python scalar, written out so that it does not
depend on the NumPy version (a float32 clip whose peak is float32(t) < t is NOT below t).  Clips of other dtypes (PCM integers) are
left to NumPy's own promotion.  A NaN sample makes a window neither quiet (< threshold) nor valid (> threshold)."""
import numpy as np
import torch

from . import clips as _clips

_DEVICE_DTYPES = (torch.float32, torch.float64)


# ------------------------------------------------------------------------------------------------------------------
# window peaks and the closed forms
# ------------------------------------------------------------------------------------------------------------------
def _sample_peaks(wave):
    """|wave| per sample: [samples, ...] -> [samples], the maximum over whatever axes follow the first"""
    a = np.abs(np.asarray(wave))
    return a.reshape(a.shape[0], -1).max(axis=1) if a.ndim > 1 else a


def _threshold(a, threshold):
    return a.dtype.type(threshold) if a.dtype.kind == "f" else threshold


def _segment(sample_rate, frame_length):
    seg = int(sample_rate * frame_length)
    if seg <= 0:
        raise ValueError("a segment of int(%r * %r) = %d samples" % (sample_rate, frame_length, seg))
    return seg


def window_peaks(a, origin, width, stride, count):
    """P[k] = max a[origin + k stride : origin + k stride + width], k < count, of a 1-D array of magnitudes (every window inside it)."""
    if count <= 0:
        return a[:0]
    return np.lib.stride_tricks.sliding_window_view(a, width)[origin::stride][:count].max(axis=1)


def tail_stop(a, thr, seg):
    """trim_tail_empty keeps a[:stop] of the magnitudes a, or nothing (None).  The windows lie on the grid that ends at n (origin
    n % seg); the walk from the last one stops at the last window that is not quiet, or at the window whose end is seg, which it never
    tests; L is where it stops."""
    n = a.shape[0]
    if n < seg:
        return None
    m, r = divmod(n, seg)
    active = np.flatnonzero(~(window_peaks(a, r, seg, seg, m) < thr))
    k = int(active[-1]) if active.size else -1
    if r == 0:
        k = max(k, 0)
    L = r + (k + 1) * seg
    if L < seg:
        return None
    return n if L == n else L - seg


def head_start(a, m, thr, seg):
    """trim_head_empty keeps a[start:m] of the first m magnitudes, or nothing (None).  The walk from 0 stops at the first window
    [k seg, (k + 1) seg) that is not quiet or at the first k seg that is not < m - seg."""
    kq = (m - 1) // seg if m > seg else 0
    active = np.flatnonzero(~(window_peaks(a, 0, seg, seg, kq) < thr))
    s = (int(active[0]) if active.size else kq) * seg
    if s >= m - seg:
        return None
    return 0 if s == 0 else s - seg


def trim_bounds(wave, threshold=500, sample_rate=44100, frame_length=0.02, which="both"):
    """(start, stop) of what trim_tail_empty ("tail"), trim_head_empty ("head") or trim_empty ("both") keeps of `wave`, or None."""
    if which not in ("tail", "head", "both"):
        raise ValueError("trim_bounds: which must be 'tail', 'head' or 'both', got %r" % (which,))
    seg = _segment(sample_rate, frame_length)
    a = _sample_peaks(wave)
    thr = _threshold(a, threshold)
    start, stop = 0, a.shape[0]
    if which != "head":
        stop = tail_stop(a, thr, seg)
        if stop is None:
            return None
    if which != "tail":
        start = head_start(a, stop, thr, seg)
        if start is None:
            return None
    return start, stop


# ------------------------------------------------------------------------------------------------------------------
# the reference's functions, one clip on the host
# ------------------------------------------------------------------------------------------------------------------
def _cut(wave, bounds):
    return None if bounds is None else wave[bounds[0]:bounds[1], ...]


def trim_tail_empty(wave, threshold=500, sample_rate=44100, frame_length=0.02):
    """audio_op.py:79-91: `wave` [samples, ...] without its quiet end, in segments of int(sample_rate * frame_length) counted back from
    the end; None for a clip shorter than a segment or quiet down to its first (partial) segment."""
    if wave is None:
        return None
    return _cut(wave, trim_bounds(wave, threshold, sample_rate, frame_length, "tail"))


def trim_head_empty(wave, threshold=500, sample_rate=44100, frame_length=0.02):
    """audio_op.py:93-105: `wave` without its quiet start, one quiet segment kept; None when no active segment starts before
    len - segment."""
    if wave is None:
        return None
    return _cut(wave, trim_bounds(wave, threshold, sample_rate, frame_length, "head"))


def trim_empty(wave, threshold=500, sample_rate=44100, frame_length=0.02):
    """audio_op.py:107-109: trim_head_empty(trim_tail_empty(wave))."""
    if wave is None:
        return None
    return _cut(wave, trim_bounds(wave, threshold, sample_rate, frame_length, "both"))


def has_long_empty(wave, length=3, sample_rate=44100, threshold=400):
    """audio_op.py:118-126: whether a window of int(sample_rate * length) samples that ends at n, n - sample_rate, ... (while it starts
    after sample 0) has a peak < threshold (the reference's 400)."""
    if wave is None:
        return None
    seg, step = _segment(sample_rate, length), int(sample_rate)
    if step <= 0:
        raise ValueError("has_long_empty: a step of %d samples" % step)
    a = _sample_peaks(wave)
    n = a.shape[0]
    count = (n - seg - 1) // step + 1 if n > seg else 0
    origin = n - seg - (count - 1) * step
    return bool((window_peaks(a, origin, seg, step, count) < _threshold(a, threshold)).any())


def is_valid_signal(wave, threshold=1000):
    """audio_op.py:149-150"""
    wave = np.asarray(wave)
    return np.max(np.abs(wave)) > _threshold(wave, threshold)


def active_frames_count(n, sample_rate=44100, frame_length=0.02, frame_shift=0.01):
    """The number of labels of a clip of n samples"""
    frame, shift = int(frame_length * sample_rate), int(frame_shift * sample_rate)
    return (n + 2 * shift - frame) // shift + 1 if n + 2 * shift >= frame else 0


def get_all_active_segment_index(wave, threshold=500, sample_rate=44100, frame_length=0.02, frame_shift=0.01):
    """audio_op.py:128-147: the clip [samples] reflect-padded by int(frame_shift * sample_rate) on both sides (librosa's pad_center
    is np.pad with (size - n) // 2 on the left), one label per frame of int(frame_length * sample_rate) samples every shift: 1 where
    is_valid_signal(frame, threshold), else 0.  -> list of ints."""
    wave = np.asarray(wave)
    frame, shift = int(frame_length * sample_rate), int(frame_shift * sample_rate)
    if wave.ndim != 1 or frame <= 0 or shift <= 0:
        raise ValueError("get_all_active_segment_index: a single channel [samples] and frames of at least one sample, got %s, %d / %d"
                         % (wave.shape, frame, shift))
    a = np.abs(np.pad(wave, shift, mode="reflect"))
    count = active_frames_count(wave.shape[0], sample_rate, frame_length, frame_shift)
    return (window_peaks(a, 0, frame, shift, count) > _threshold(a, threshold)).astype(int).tolist()


def max_mag_unify(ref, est):
    """audio_op.py:71-77: est scaled to ref's peak -> (ref, est * (max |ref| / max |est|))."""
    max_val_ref = np.max(np.abs(ref))
    max_val_est = np.max(np.abs(est))
    return ref, est * (max_val_ref / max_val_est)


# ------------------------------------------------------------------------------------------------------------------
# list forms: padded batches on the device
# ------------------------------------------------------------------------------------------------------------------
def _engine(engine):
    from . import simulate
    return simulate._engine_or_default(engine)


def _device_dtype(c, longer_than=0):
    """The torch dtype of a clip the kernels take -- 1-D, float32 or float64, more than `longer_than` samples -- or None"""
    if len(list(c.shape)) != 1 or c.shape[0] <= longer_than:
        return None
    for dtype in _DEVICE_DTYPES:
        if str(c.dtype).endswith(str(dtype).split(".")[-1]):
            return dtype
    return None


def _device_batches(clips, engine, longer_than=0):
    """The clips the kernels take, as padded batches: yields (eng, idx, x (len(idx), ld), lens) per dtype and batch of up to MAX_BATCH
    clips sorted by length, rows padded to a multiple of 4 samples (the kernels' 16-byte accesses)."""
    from .simulate import MAX_BATCH
    lengths = [c.shape[0] if len(list(c.shape)) else 0 for c in clips]
    for dtype in _DEVICE_DTYPES:
        dev = [i for i in range(len(clips)) if _device_dtype(clips[i], longer_than) == dtype]
        for idx in _clips.batches(dev, lengths, MAX_BATCH):
            eng = _engine(engine)
            lens = [lengths[i] for i in idx]
            yield eng, idx, _clips.pad([clips[i] for i in idx], eng.device, dtype, width=(lens[-1] + 3) // 4 * 4), lens


def _bounds_list(clips, which, threshold, sample_rate, frame_length, engine, rows=None):
    """[(start, stop) or None per clip]: the device for float32 / float64 clips (ONE device-to-host copy per batch), the host form for
    the rest.  `rows`, a dict, receives the padded batch's row of every clip that went to the device."""
    _segment(sample_rate, frame_length)
    out, done = [None] * len(clips), set()
    for eng, idx, x, lens in _device_batches(clips, engine):
        start, stop = eng.trim_bounds(x, lens, threshold, sample_rate, frame_length, which)
        for j, (i, s, e) in enumerate(zip(idx, *torch.stack([start, stop]).cpu().tolist())):
            out[i] = None if s < 0 else (s, e)
            done.add(i)
            if rows is not None:
                rows[i] = x[j]
    for i in range(len(clips)):
        if i not in done:
            out[i] = trim_bounds(_clips.as_numpy(clips[i]), threshold, sample_rate, frame_length, which)
    return out


def _trim_list(clips, which, threshold, sample_rate, frame_length, engine, to_host):
    clips = list(clips)
    rows = {}
    bounds = _bounds_list(clips, which, threshold, sample_rate, frame_length, engine, rows)
    out = []
    for i, b in enumerate(bounds):
        if b is None:
            out.append(None)
        elif to_host:
            out.append(_clips.as_numpy(clips[i])[b[0]:b[1], ...])
        else:
            row = rows[i] if i in rows else _clips.to_device(clips[i], _engine(engine).device)
            out.append(row[b[0]:b[1], ...])
    return out


def trim_tail_empty_list(clips, threshold=500, sample_rate=44100, frame_length=0.02, engine=None, to_host=True):
    """`trim_tail_empty` for a list of clips of any lengths (NumPy arrays or tensors, on any device) -> list in the caller's order, None
    where the host form returns None.  Non-empty 1-D float32 and float64 clips go through Engine.trim_bounds as padded batches of up
    to MAX_BATCH sorted by length -- the bounds come to the host in one copy per batch, the samples do not --, every other clip takes
    the host form.  to_host: NumPy arrays (views of NumPy inputs, as the reference returns); else device tensors (views of the batch)."""
    return _trim_list(clips, "tail", threshold, sample_rate, frame_length, engine, to_host)


def trim_head_empty_list(clips, threshold=500, sample_rate=44100, frame_length=0.02, engine=None, to_host=True):
    """`trim_head_empty` for a list of clips (cf. trim_tail_empty_list)."""
    return _trim_list(clips, "head", threshold, sample_rate, frame_length, engine, to_host)


def trim_empty_list(clips, threshold=500, sample_rate=44100, frame_length=0.02, engine=None, to_host=True):
    """`trim_empty` for a list of clips (cf. trim_tail_empty_list): the trimmed clips, None entries included."""
    return _trim_list(clips, "both", threshold, sample_rate, frame_length, engine, to_host)


def trim_empty_bounds_list(clips, threshold=500, sample_rate=44100, frame_length=0.02, engine=None):
    """What `trim_empty` keeps of every clip, as [(start, stop) or None]: one device-to-host copy per batch of up to MAX_BATCH clips."""
    return _bounds_list(list(clips), "both", threshold, sample_rate, frame_length, engine)


def has_long_empty_list(clips, length=3, sample_rate=44100, threshold=400, engine=None, to_host=True):
    """`has_long_empty` for a list of clips (batched as in trim_tail_empty_list) -> list of bools (to_host), or ONE (len(clips),) bool
    tensor on the device in the caller's order."""
    clips = list(clips)
    _segment(sample_rate, length)
    out, parts = [None] * len(clips), []
    for eng, idx, x, lens in _device_batches(clips, engine):
        flag = eng.has_long_empty(x, lens, length, sample_rate, threshold)
        if to_host:
            for i, f in zip(idx, flag.cpu().tolist()):
                out[i] = bool(f)
        else:
            parts.append((idx, flag != 0))
            for i in idx:
                out[i] = True
    rest = [i for i in range(len(clips)) if out[i] is None]
    for i in rest:
        out[i] = has_long_empty(_clips.as_numpy(clips[i]), length, sample_rate, threshold)
    if to_host:
        return out
    dev = _engine(engine).device
    res = torch.zeros((len(clips),), device=dev, dtype=torch.bool)
    if rest:
        res[torch.tensor(rest, device=dev)] = torch.tensor([out[i] for i in rest], device=dev)
    for idx, flag in parts:
        res[torch.tensor(idx, device=dev)] = flag
    return res


def active_frames_list(clips, threshold=500, sample_rate=44100, frame_length=0.02, frame_shift=0.01, engine=None, to_host=True):
    """`get_all_active_segment_index` for a list of clips -> per clip its labels: a list of ints (to_host: one copy per batch), or a
    uint8 tensor on the device.  1-D float32 and float64 clips of more than int(frame_shift * sample_rate) samples -- one reflection --
    go through Engine.active_frames, batched as in trim_tail_empty_list; every other clip takes the host form."""
    clips = list(clips)
    shift = int(frame_shift * sample_rate)
    out = [None] * len(clips)
    for eng, idx, x, lens in _device_batches(clips, engine, longer_than=max(shift, 0)):
        labels, counts = eng.active_frames(x, lens, threshold, sample_rate, frame_length, frame_shift)
        counts = [active_frames_count(n, sample_rate, frame_length, frame_shift) for n in lens]
        if to_host:
            labels = labels.cpu().numpy()
        for j, i in enumerate(idx):
            out[i] = labels[j, :counts[j]].astype(int).tolist() if to_host else labels[j, :counts[j]]
    for i in range(len(clips)):
        if out[i] is None:
            y = get_all_active_segment_index(_clips.as_numpy(clips[i]), threshold, sample_rate, frame_length, frame_shift)
            out[i] = y if to_host else torch.tensor(y, device=_engine(engine).device, dtype=torch.uint8)
    return out


def max_mag_unify_list(refs, ests, engine=None, to_host=True):
    """`max_mag_unify` for lists of clips -> (refs, [est * (max |ref| / max |est|)]).  Pairs of non-empty 1-D clips of ONE dtype,
    float32 or float64, run on the device as padded batches: the peaks are those of the clip-batch layer (Engine.quantize returns
    max |x| of every clip in the clip's dtype), their quotient and the one multiplication per sample are element-wise operations in
    that dtype -- bit for bit the host form.  Every other pair takes the host form.  `refs` comes back as it was given."""
    refs, ests = list(refs), list(ests)
    if len(refs) != len(ests):
        raise ValueError("max_mag_unify_list: %d refs for %d ests" % (len(refs), len(ests)))
    paired = [e if _device_dtype(e) is not None and _device_dtype(r) == _device_dtype(e) else np.zeros((0,)) for r, e in zip(refs, ests)]
    out = [None] * len(ests)
    for eng, idx, x, lens in _device_batches(paired, engine):
        rlens = [refs[i].shape[0] for i in idx]
        r = _clips.pad([refs[i] for i in idx], eng.device, x.dtype, width=(max(rlens) + 3) // 4 * 4)
        ratio = eng.quantize(r, 0, lengths=rlens)[1] / eng.quantize(x, 0, lengths=lens)[1]
        for i, row in zip(idx, _clips.unpad(x * ratio[:, None], lens, to_host)):
            out[i] = row
    for i in range(len(ests)):
        if out[i] is None:
            y = max_mag_unify(_clips.as_numpy(refs[i]), _clips.as_numpy(ests[i]))[1]
            out[i] = y if to_host else _clips.to_device(y, _engine(engine).device)
    return refs, out
