"""NumPy model of a streaming session (TEST INFRASTRUCTURE; nothing under voicefixer_main_amd/ imports it).

What `vfx_stream_*` does, restated on the host: an input ring, an accumulator ring and an output ring per slot, all addressed
`n % capacity`; the schedule of the issue (which chunk is due when, the order of the rows of a group, back-pressure); the
overlap-add sum in float32, ascending k, one fused multiply-add per term as `k_chunk_ola` compiles it.  Every call appends one line
to `log`: the schedule, in the very format tests/stream_sched_main.cpp prints for the library's own scheduler.

`drive()` plays the caller: it feeds seeded blockings the way StreamRestorer.feed does and records every call it made (`ops`), so
that the same calls can be replayed against stream_sched.cpp.

`defect=` plants one fault (the tests show that each moves a sample's bits or the counts):
  "descending"  a group's chunks of a slot are accumulated in descending k
  "no_clear"    the accumulator is not cleared when a slot is opened again
  "no_fill"     at close, samples past the end are read from the ring instead of being zero
  "wrap"        the input ring wraps one cell late
  "back_margin" the last boxcar frame is run with a back margin
"""
import numpy as np

OLA, BOXCAR = 0, 1
BLOCK_SIZES = lambda W, H: (0, 1, 3, H - 1, H, H + 1, W, 2 * W + 5)   # noqa: E731  (the issue's block sizes)


def fma32(a, b, c):
    """float32 a * b + c with one rounding (the product of two float32 is exact in float64; the float64 sum is then rounded to
    float32 -- a second rounding that can differ from a true FMA only at a float64 tie, which tolerances of 1e-6 do not see)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def released_before_close(mode, W, P, n):
    """The issue's two formulas: samples a slot has released after n fed samples, before close."""
    if mode == OLA:
        return max(0, (n // P + 1) * P - W)
    return W * ((n - P) // W) if n >= W + P else 0


class Refused(Exception):
    pass


class StreamModel:
    def __init__(self, slots, mode, W, P, window, scale, cap_in, cap_out, defect=None):
        assert W % 2 == 0 and (1 <= P <= W if mode == OLA else P >= 0)
        assert cap_in >= (W if mode == OLA else W + 2 * P) and cap_out >= W
        self.S, self.mode, self.W, self.P = slots, mode, W, P
        self.window = None if window is None else np.asarray(window, np.float32)
        self.scale = np.float32(scale)
        self.cap_in, self.cap_out = cap_in, cap_out
        self.cap_acc = cap_in + 3 * W          # holds the longest span one group can touch: what one push holds plus the flush
        self.defect = defect
        self.ring = np.zeros((slots, cap_in + 1), np.float32)   # one spare cell: where the planted late wrap lands
        self.acc = np.zeros((slots, self.cap_acc), np.float32)
        self.out = np.zeros((slots, cap_out), np.float32)
        self.st = [dict(state="free", fed=0, consumed=0, next=0, released=0, popped=0) for _ in range(slots)]
        self.group = None
        self.log = []

    # ------------------------------------------------------------------ the schedule
    def _due(self, s, k):
        """Chunk k of slot state s, if it is due: dict(start, len, off, count, n0, final_end, release_end, consumed_after)."""
        W, P, L = self.W, self.P, s["fed"]
        closing = s["state"] == "closing"
        if s["state"] not in ("open", "closing"):
            return None
        if self.mode == OLA:
            k_last = (L + W - 1) // P
            if (closing and not (L > 0 and k <= k_last)) or (not closing and L < k * P):
                return None
            last = closing and k == k_last
            nxt = max(0, (k + 1) * P - W)
            return dict(start=k * P - W, len=W, final_end=k * P if last else nxt, release_end=L if last else nxt, consumed_after=nxt)
        nch = -(-L // W)
        if (closing and k >= nch) or (not closing and L < (k + 1) * W + P):
            return None
        tail = L % W
        if k == 0:
            c = dict(start=0, len=W + P, off=0, count=min(W, L) if closing else W)
        elif closing and k == nch - 1:
            c = dict(start=k * W - P, len=P + (tail or W) + (P if self.defect == "back_margin" else 0), off=P, count=tail or W)
        else:
            c = dict(start=k * W - P, len=W + 2 * P, off=P, count=W)
        c.update(n0=k * W, release_end=k * W + c["count"], consumed_after=max(0, (k + 1) * W - P))
        return c

    def open(self):
        for i, s in enumerate(self.st):
            if s["state"] == "free" or (s["state"] == "closed" and s["popped"] == s["released"]):
                s.update(state="open", fed=0, consumed=0, next=1 if self.mode == OLA else 0, released=0, popped=0)
                if self.defect != "no_clear":
                    self.acc[i] = 0
                self.log.append("open %d" % i)
                return i
        raise Refused("open: all slots are in use")

    def room(self, slot):
        s = self.st[slot]
        return self.cap_in - (s["fed"] - s["consumed"]) if s["state"] == "open" else 0

    def push(self, blocks):
        """blocks: [(slot, array)].  Refused as a whole, before anything is copied."""
        for i, (slot, b) in enumerate(blocks):
            if self.st[slot]["state"] != "open":
                self.log.append("push refused")
                raise Refused("push: slot %d is not open" % slot)
            if len(b) > self.room(slot) or slot in [q for q, _ in blocks[:i]]:
                self.log.append("push refused")
                raise Refused("push: overrun of slot %d" % slot)
        rows, off = [], 0
        for slot, b in blocks:
            s, n = self.st[slot], len(b)
            if n:
                pos = s["fed"] % self.cap_in
                rows.append("%d:%d:%d:%d" % (slot, off, n, pos))
                self.ring[slot, self._cells(pos, n)] = b
            s["fed"] += n
            off += n
        self.log.append(" ".join(["push"] + rows))

    def _cells(self, pos, n, reading=False):
        c = pos + np.arange(n)
        late = reading and self.defect == "wrap"
        return np.where(c > self.cap_in if late else c >= self.cap_in, c - self.cap_in, c)

    def close(self, slot):
        s = self.st[slot]
        if s["state"] != "open":
            raise Refused("close: slot %d is not open" % slot)
        s["state"] = "closing"
        if not (self.group and any(r[0] == slot for r in self.group)) and self._due(s, s["next"]) is None:
            s["state"] = "closed"
        self.log.append("close %d" % slot)

    def next(self, max_rows):
        """-> (rows, row_len) chunk batch of the due chunks: by slot, then ascending k, one row length per group."""
        if self.group:
            raise Refused("next: the previous group has not been put")
        group, row_len = [], 0
        for i, s in enumerate(self.st):
            while len(group) < max_rows:
                c = self._due(s, s["next"])
                if c is None or c["release_end"] - s["popped"] > self.cap_out or (row_len and c["len"] != row_len):
                    break
                row_len = c["len"]
                group.append((i, s["next"], c, s["fed"]))
                s["consumed"] = c["consumed_after"]
                s["next"] += 1
        if not group:
            self.log.append("next 0")
            return np.zeros((0, 0), np.float32)
        chunks = np.zeros((len(group), row_len), np.float32)
        rows = []
        for r, (i, k, c, valid_end) in enumerate(group):
            n = c["start"] + np.arange(row_len)
            closing = self.st[i]["state"] == "closing"
            live = (n >= 0) & ((n < valid_end) | (closing and self.defect == "no_fill"))
            pos = c["start"] % self.cap_in
            chunks[r, live] = self.ring[i, self._cells(pos, row_len, reading=True)[live]]
            rows.append("%d:%d:%d:%d" % (i, c["start"], valid_end, pos))
        self.group = [(i, k, c) for i, k, c, _ in group]
        self.log.append(" ".join(["next %d" % row_len] + rows))
        return chunks

    def put(self, frames):
        if not self.group:
            raise Refused("put: no group is outstanding")
        frames = np.asarray(frames, np.float32)
        assert frames.shape[0] == len(self.group) and frames.shape[1] == self.group[0][2]["len"]
        W, P = self.W, self.P
        rows, a = [], 0
        while a < len(self.group):
            b = a
            while b < len(self.group) and self.group[b][0] == self.group[a][0]:
                b += 1
            i, s = self.group[a][0], self.st[self.group[a][0]]
            last = self.group[b - 1][2]
            if self.mode == OLA:
                order = range(b - 1, a - 1, -1) if self.defect == "descending" else range(a, b)
                for r in order:
                    k = self.group[r][1]
                    n = k * P - W + np.arange(W)
                    keep = n >= 0
                    cells = n[keep] % self.cap_acc
                    w = self.window[keep] if self.window is not None else self.scale
                    self.acc[i, cells] = fma32(frames[r, keep], w, self.acc[i, cells])
                n = np.arange(s["released"], last["release_end"])           # final now: to the output ring, cells cleared
                self.out[i, n % self.cap_out] = self.acc[i, n % self.cap_acc]
                self.acc[i, n % self.cap_acc] = 0
                k0, k1 = self.group[a][1], self.group[b - 1][1]
                rows.append("%d:%d:%d:%d:%d:%d:%d:%d" % (i, a, b - a, k0, max(0, k0 * P - W), k1 * P, last["final_end"],
                                                         last["release_end"]))
            else:
                for r in range(a, b):
                    c = self.group[r][2]
                    f = frames[r, c["off"]:c["off"] + c["count"]]
                    w = self.window[:c["count"]] if self.window is not None else self.scale
                    self.out[i, (c["n0"] + np.arange(c["count"])) % self.cap_out] = fma32(f, w, np.float32(0))
                    rows.append("%d:%d:%d:%d:%d" % (i, r, c["off"], c["count"], c["n0"]))
            s["released"] = max(s["released"], last["release_end"])
            if s["state"] == "closing" and self._due(s, s["next"]) is None:
                s["state"] = "closed"
            a = b
        self.group = None
        self.log.append(" ".join(["put"] + rows))

    def available(self, slot):
        return self.st[slot]["released"] - self.st[slot]["popped"]

    def state(self, slot):
        s = self.st[slot]
        self.log.append("state %d %d %d %d %d" % (slot, s["fed"], s["released"], self.available(slot), self.room(slot)))
        return s["fed"], s["released"]

    def pop(self, slots):
        """Everything released of `slots` -> list of arrays."""
        res, rows, off = [], [], 0
        for slot in slots:
            s = self.st[slot]
            n = self.available(slot)
            if n:
                rows.append("%d:%d:%d:%d" % (slot, off, n, s["popped"] % self.cap_out))
            res.append(self.out[slot, (s["popped"] + np.arange(n)) % self.cap_out].copy())
            s["popped"] += n
            off += n
        self.log.append(" ".join(["pop"] + rows))
        return res


# ---------------------------------------------------------------------------------------------------------------------------------
# the caller
# ---------------------------------------------------------------------------------------------------------------------------------
def blocking(rng, lengths, sizes):
    """A seeded interleaved blocking of streams of `lengths`: a list of events {stream index: block size}; every stream gets all
    of its samples, in blocks drawn from `sizes` (the last block of a stream is cut to what is left)."""
    left = list(lengths)
    events = []
    while any(left):
        ev = {}
        for j, rest in enumerate(left):
            if rest and rng.random() < 0.6:
                ev[j] = min(rest, int(sizes[rng.integers(len(sizes))]))
                left[j] -= ev[j]
        if ev:
            events.append(ev)
    return events


def drive(model, nnet, signals, events, max_rows=64, ops=None, after_feed=None):
    """Feed `signals` (a list of 1-D arrays) to slots opened in that order, block by block as `events` says, the way
    StreamRestorer.feed does; then close them in order.  -> the concatenated output of every signal.
    ops: a list that receives every call as the text line stream_sched_main reads.  after_feed(slot, fed, released)."""
    ops = [] if ops is None else ops

    def step():
        any_group = False
        while True:
            ops.append("N %d" % max_rows)
            chunks = model.next(max_rows)
            if not len(chunks):
                return any_group
            any_group = True
            model.put(nnet(chunks[:, None, :])[:, 0, :])

    def pop(slots, out):
        if not any(model.available(s) for s in slots):
            return False
        ops.append("G %d %s" % (len(slots), " ".join(map(str, slots))))
        for s, piece in zip(slots, model.pop(slots)):
            out[s].append(piece)
        return True

    slot_of = []
    for _ in signals:
        ops.append("O")
        slot_of.append(model.open())
    out = {s: [] for s in slot_of}
    done = [0] * len(signals)
    for ev in events:
        streams = list(ev)
        slots = [slot_of[j] for j in streams]
        want = dict(ev)
        first = True
        while True:
            counts = [min(want[j], model.room(slot_of[j])) for j in streams]
            if sum(counts) or first:
                ops.append("P %d %s" % (len(slots), " ".join("%d %d" % sc for sc in zip(slots, counts))))
                model.push([(slot_of[j], signals[j][done[j]:done[j] + c]) for j, c in zip(streams, counts)])
                for j, c in zip(streams, counts):
                    done[j] += c
                    want[j] -= c
                first = False
            stepped = step()
            if not (pop(slots, out) or stepped or sum(counts)):
                break
        assert not any(want.values())
        for s in slots:
            ops.append("R %d" % s)
            fed, released = model.state(s)
            if after_feed:
                after_feed(s, fed, released)
    for j, s in enumerate(slot_of):
        assert done[j] == len(signals[j])
        ops.append("C %d" % s)
        model.close(s)
        while True:
            stepped = step()
            if not (pop([s], out) or stepped):
                break
        ops.append("R %d" % s)
        model.state(s)
    return [np.concatenate(out[s]) if out[s] else np.zeros(0, np.float32) for s in slot_of]
