"""Streaming sessions: the two long-audio chunkers of chunker.py for audio that arrives in blocks.

`StreamRestorer` holds `slots` independent mono streams.  A caller opens a slot, feeds it blocks of whatever size its source
delivers and gets back, block by block, every output sample that no later chunk can change; closing the slot flushes the tail.
Fed in ANY blocking, and beside any other streams, the concatenated output of a slot is bit for bit what `LambdaOverlapAdd`
(with `hop_size`) or `LambdaOverlapAddBoxcar` (with `in_margin`) returns for the whole signal: the offline classes define the
semantics and nothing else is ever computed.

All audio state lives on the device in libvfx (`vfx_stream_*`): an input ring and an output ring per slot and, in overlap-add
mode, the partial sums of the span later chunks still add to.  The library works out on the host, from sample counts alone, which
chunk of which slot is due; the due chunks of ALL slots come back as one batch per row length, so `nnet` runs once per step however
many streams are live.  As with the chunkers the network call stays here: `nnet(x: (N, 1, n)) -> {key: (N, 1, n)}`.

Before close, a slot fed n samples has released max(0, (n // hop + 1) * hop - window_size) samples in overlap-add mode and
window_size * ((n - in_margin) // window_size) (0 below window_size + in_margin) in boxcar mode; after close, all n.
"""
import numpy as np
import torch

from . import _lib
from .chunker import _window


class StreamRestorer:
    def __init__(self, nnet, window_size, hop_size=None, in_margin=None, window="hanning", slots=16, capacity=None, max_batch=64,
                 engine=None, key="wav"):
        if in_margin is not None and hop_size is not None:
            raise ValueError("in_margin selects the boxcar chunker, which has no hop_size: give one of the two")
        if window_size % 2 != 0:
            raise ValueError("Window size must be even")
        self.nnet = nnet
        self.key = key
        self.engine = engine if engine is not None else getattr(nnet, "engine", None)
        if self.engine is None:
            raise ValueError("no libvfx engine: pass engine= or an nnet that carries one")
        self.device = self.engine.device
        self.window_size = int(window_size)
        self.boxcar = in_margin is not None
        if self.boxcar:
            self.in_margin, self.hop_size = int(in_margin), self.window_size
            mode, par, scale = _lib.STREAM_BOXCAR, self.in_margin, 1.0
            longest = self.window_size + 2 * self.in_margin
        else:
            self.in_margin, self.hop_size = None, int(hop_size) if hop_size is not None else self.window_size // 2
            mode, par, scale = _lib.STREAM_OLA, self.hop_size, 1.0 / (self.window_size / self.hop_size)
            longest = self.window_size
        # default: two chunks' worth, on the 16-byte grid that the vector gather needs
        self.capacity = int(capacity) if capacity is not None else (2 * longest + 3) // 4 * 4
        self.max_batch = int(max_batch)
        if self.max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        self.slots = int(slots)
        win = torch.from_numpy(_window(window, self.window_size)).to(self.device) if window else None
        self._st = self.engine.stream_create(self.slots, mode, self.window_size, par, win, scale, self.capacity,
                                             max(self.capacity, self.window_size))
        self._chunks = torch.empty(self.max_batch * longest, device=self.device, dtype=torch.float32)

    # ------------------------------------------------------------------ the session
    def open(self):
        """A free slot (a closed slot is free again once its tail has been returned)."""
        return self.engine.stream_open(self._st)

    def state(self, slot):
        """(samples fed, samples released) of the slot's stream."""
        return self.engine.stream_state(self._st, slot)

    def feed(self, blocks):
        """blocks: {slot: 1-D float32 array or tensor, host or device} -> {slot: device tensor of the samples that became final}.
        A block of any size, zero included; what does not fit the input ring at once goes in pieces."""
        slots = list(blocks)
        data = {}
        for s in slots:
            b = blocks[s]
            if not isinstance(b, torch.Tensor):
                b = torch.as_tensor(np.asarray(b, dtype=np.float32))
            if b.dim() != 1:
                raise ValueError("feed: the block of slot %d must be 1-D, got %s" % (s, tuple(b.shape)))
            data[s] = b.to(device=self.device, dtype=torch.float32)
        done = dict.fromkeys(slots, 0)
        out = {s: [] for s in slots}
        first = True
        with torch.no_grad():
            while True:
                counts = [min(data[s].numel() - done[s], self.engine.stream_room(self._st, s)) for s in slots]
                pushed = sum(counts)
                if pushed or first:   # an empty feed still reaches the library: a closed slot is refused there
                    pieces = [data[s][done[s]:done[s] + c] for s, c in zip(slots, counts)]
                    self.engine.stream_push(self._st, slots, counts, torch.cat(pieces).contiguous() if pieces else None)
                    for s, c in zip(slots, counts):
                        done[s] += c
                    first = False
                stepped = self._step()
                popped = self._pop(slots, out)
                if not (pushed or stepped or popped):
                    break
        left = [s for s in slots if done[s] < data[s].numel()]
        if left:
            raise RuntimeError("feed: the input ring of slot %d takes no more samples although nothing is due" % left[0])
        return {s: self._join(out[s]) for s in slots}

    def close(self, slot):
        """End the slot's stream -> its tail: every sample not yet returned.  The slot can be opened again afterwards."""
        self.engine.stream_close(self._st, slot)
        out = {slot: []}
        with torch.no_grad():
            while True:
                stepped = self._step()
                if not (self._pop([slot], out) or stepped):
                    break
        return self._join(out[slot])

    def shutdown(self):
        if getattr(self, "_st", None) is not None and getattr(self.engine, "h", None):
            self.engine.stream_destroy(self._st)
        self._st = None

    def __del__(self):
        try:
            self.shutdown()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _step(self):
        """Run every group that is due: one nnet call per group.  -> whether there was one."""
        any_group = False
        while True:
            rows, row_len = self.engine.stream_next(self._st, self.max_batch, self._chunks)
            if rows == 0:
                return any_group
            any_group = True
            frame = self.nnet(self._chunks[:rows * row_len].view(rows, 1, row_len))[self.key]
            assert frame.ndim == 3, "nnet should return (batch, n_src, time)"
            if frame.shape[1] != 1:
                raise NotImplementedError("nnet returned %d sources; one is supported" % frame.shape[1])
            if frame.shape[0] != rows or frame.shape[2] != row_len:
                raise ValueError("nnet returned %s for %d chunks of %d samples" % (tuple(frame.shape), rows, row_len))
            self.engine.stream_put(self._st, frame.to(torch.float32).reshape(rows, row_len).contiguous())

    def _pop(self, slots, out):
        """Everything released of `slots` onto their lists -> whether there was anything."""
        some = False
        for s, piece in zip(slots, self.engine.stream_pop(self._st, slots, [self.capacity + self.window_size] * len(slots))):
            if piece.numel():
                out[s].append(piece)
                some = True
        return some

    def _join(self, pieces):
        if not pieces:
            return torch.empty(0, device=self.device, dtype=torch.float32)
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces)
