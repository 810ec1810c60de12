"""GPU: streaming sessions (voicefixer_main_amd/streaming.py, vfx_stream_*, stream.hip) against the offline chunkers.

The oracle is exact: fed in any blocking and beside any other streams, a slot's concatenated output is `torch.equal` to what
`LambdaOverlapAdd` / `LambdaOverlapAddBoxcar` return for the whole signal.  Shapes, lengths and block sizes are the issue's; the
seeded blockings are those of tests/stream_ref.py.  The stand-in network is the device copy of oracle.chunker.toy_nnet; because that
one is causal (what a chunk holds past the end of its stream never reaches a kept sample), the zero fill at close is also run
through its mirror image, which looks one sample ahead.
"""
import numpy as np
import pytest
import torch

import stream_ref as sr

pytestmark = pytest.mark.gpu

LENGTHS = (1237, 64, 5)
# (mode, W, hop or margin, window, ring capacity): every ring wraps many times in 1237 samples.  100 keeps rows on the 16-byte grid
# (vector gather); the odd capacities take the scalar path.
SHAPES = [
    (sr.OLA, 64, 16, "hanning", 100),
    (sr.OLA, 64, 32, None, 64 + 37),
    (sr.OLA, 126, 21, None, 126 + 37),
    (sr.BOXCAR, 64, 8, "hanning", 64 + 16 + 37),
    (sr.BOXCAR, 126, 7, None, 126 + 14 + 37),
]
IDS = ["%s-%d-%d-%s" % ("ola" if m == sr.OLA else "box", W, P, w) for m, W, P, w, _ in SHAPES]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd.engine import Engine
    return Engine("cuda:0")


def _toy_net(x):
    """oracle.chunker.toy_nnet as device code."""
    prev = torch.cat([torch.zeros_like(x[..., :1]), x[..., :-1]], -1)
    n = x.shape[-1]
    ramp = (torch.arange(n, dtype=torch.float32, device=x.device) / n) * 0.05
    return {"wav": 0.6 * x + 0.3 * prev + ramp}


def _lookahead_net(x):
    """_toy_net mirrored in time: every output sample depends on the next input sample."""
    return {"wav": _toy_net(x.flip(-1))["wav"].flip(-1)}


def _signals(seed, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32)).cuda() for n in lengths]


def _offline(eng, mode, W, P, win, x, nnet=_toy_net, max_batch=64):
    from voicefixer_main_amd.chunker import LambdaOverlapAdd, LambdaOverlapAddBoxcar
    if mode == sr.OLA:
        m = LambdaOverlapAdd(nnet, 1, W, hop_size=P, window=win, engine=eng, max_batch=max_batch)
    else:
        m = LambdaOverlapAddBoxcar(nnet, 1, W, P, window=win, engine=eng, max_batch=max_batch)
    return m(x[None, None])[0, 0]


def _restorer(eng, mode, W, P, win, capacity, slots=4, nnet=_toy_net, max_batch=64):
    from voicefixer_main_amd.streaming import StreamRestorer
    kw = dict(hop_size=P) if mode == sr.OLA else dict(in_margin=P)
    return StreamRestorer(nnet, W, window=win, slots=slots, capacity=capacity, max_batch=max_batch, engine=eng, **kw)


def _play(r, signals, slots, events, mode, W, P, host_blocks=False):
    """Feed signals[j] to slots[j] block by block as `events` says, then close them -> the concatenated output of every signal.
    After every feed: what came back is what the released count grew by, the count is the issue's formula, state() agrees."""
    out = [[] for _ in signals]
    done = [0] * len(signals)
    for ev in events:
        blocks = {}
        for j, n in ev.items():
            b = signals[j][done[j]:done[j] + n]
            blocks[slots[j]] = b.cpu().numpy() if host_blocks else b
            done[j] += n
        got = r.feed(blocks)
        assert set(got) == set(blocks)
        for j in ev:
            piece = got[slots[j]]
            assert piece.device.type == "cuda" and piece.dtype == torch.float32 and piece.dim() == 1
            out[j].append(piece)
            fed, released = r.state(slots[j])
            assert fed == done[j]
            assert released == sr.released_before_close(mode, W, P, fed) == sum(p.numel() for p in out[j]), (j, fed, released)
    res = []
    for j, s in enumerate(slots):
        assert done[j] == signals[j].numel()
        out[j].append(r.close(s))
        assert r.state(s) == (done[j], done[j])
        res.append(torch.cat(out[j]))
    return res


def _events(seed, W, P, mode, lengths=LENGTHS):
    return sr.blocking(np.random.default_rng(seed), list(lengths), sr.BLOCK_SIZES(W, P if mode == sr.OLA else max(P, 2)))


@pytest.mark.parametrize("mode,W,P,win,cap", SHAPES, ids=IDS)
def test_stream_equals_offline_chunker_in_any_blocking_and_company(eng, mode, W, P, win, cap):
    """Tests 1-3 of the issue: three of four slots carry 1237, 64 and 5 samples in an interleaved seeded blocking; the same signals
    in a second blocking on other slots (host blocks this time) beside a slot that sits idle with half a chunk; and each alone in a
    one-slot session.  Every output is bit for bit the offline chunker's; the released counts hold after every feed."""
    signals = _signals(11)
    ref = [_offline(eng, mode, W, P, win, x) for x in signals]
    # first blocking: slots 0, 1, 3 of four
    r = _restorer(eng, mode, W, P, win, cap)
    opened = [r.open() for _ in range(4)]
    assert opened == [0, 1, 2, 3]
    got = _play(r, signals, [0, 1, 3], _events(21, W, P, mode), mode, W, P)
    for y, want in zip(got, ref):
        assert y.shape == want.shape and torch.equal(y, want)
    assert r.state(2) == (0, 0) and r.close(2).numel() == 0        # fed nothing: runs nothing, releases nothing
    r.shutdown()
    # second blocking, other slots, an idle neighbour
    r = _restorer(eng, mode, W, P, win, cap)
    for _ in range(4):
        r.open()
    idle = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, 2 * W + 9).astype(np.float32)).cuda()
    few = (P if mode == sr.OLA else W + P) - 1                       # one sample short of its first chunk
    assert r.feed({0: idle[:few]})[0].numel() == 0
    got = _play(r, signals, [3, 2, 1], _events(22, W, P, mode), mode, W, P, host_blocks=True)
    for y, want in zip(got, ref):
        assert torch.equal(y, want)
    assert r.state(0) == (few, 0)
    tail = torch.cat([r.feed({0: idle[few:]})[0], r.close(0)])
    assert torch.equal(tail, _offline(eng, mode, W, P, win, idle))
    r.shutdown()
    # alone
    for x, want in zip(signals, ref):
        r = _restorer(eng, mode, W, P, win, cap, slots=1)
        assert r.open() == 0
        y = _play(r, [x], [0], _events(23, W, P, mode, [x.numel()]), mode, W, P)[0]
        assert torch.equal(y, want)
        r.shutdown()


@pytest.mark.parametrize("mode,W,P,win,cap", [SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[4]], ids=[IDS[0], IDS[2], IDS[3], IDS[4]])
def test_zero_fill_at_close_and_slot_reuse(eng, mode, W, P, win, cap):
    """Test 4: a slot is closed, opened again and fed another signal -- no residue of the first, in the rings or the accumulator.
    The network looks one sample ahead, so every sample next to the end of a stream shows what its chunk held past that end; the
    second streams are shorter than a frame, whose zero fill lies over the first stream's samples in the ring."""
    r = _restorer(eng, mode, W, P, win, cap, slots=2, nnet=_lookahead_net)
    first = _signals(31, (1237, 3 * W + 3))
    again = _signals(32, (5, W - 1))
    for signals, seed in ((first, 41), (again, 42), (first[::-1], 43)):
        slots = [r.open(), r.open()]
        assert slots == [0, 1]
        lengths = [x.numel() for x in signals]
        got = _play(r, signals, slots, _events(seed, W, P, mode, lengths), mode, W, P)
        for x, y in zip(signals, got):
            assert torch.equal(y, _offline(eng, mode, W, P, win, x, nnet=_lookahead_net)), (seed, x.numel())
    r.shutdown()


def test_many_slots(eng):
    """Test 5: 130 slots, W = 16, H = 8, lengths 20 to 60: launch tables longer than one launch takes, groups cut at max_batch."""
    from voicefixer_main_amd.chunker import LambdaOverlapAdd
    W, H, S = 16, 8, 130
    rng = np.random.default_rng(51)
    lengths = [20 + (7 * i) % 41 for i in range(S)]
    signals = [torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32)).cuda() for n in lengths]
    r = _restorer(eng, sr.OLA, W, H, "hanning", 24, slots=S)
    slots = [r.open() for _ in range(S)]
    assert slots == list(range(S))
    events = []
    for t in range(0, 60, 7):       # all streams in step, 7 samples at a time
        ev = {j: min(7, lengths[j] - t) for j in range(S) if lengths[j] > t}
        events.append(ev)
    got = _play(r, signals, slots, events, sr.OLA, W, H)
    off = LambdaOverlapAdd(_toy_net, 1, W, hop_size=H, window="hanning", engine=eng)
    for n in sorted(set(lengths)):   # the offline chunker once per length, all signals of that length as its batch
        idx = [j for j in range(S) if lengths[j] == n]
        want = off(torch.stack([signals[j] for j in idx])[:, None])
        for row, j in enumerate(idx):
            assert torch.equal(got[j], want[row, 0]), j
    r.shutdown()


@pytest.mark.parametrize("mode,W,P,win,cap", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_grouping_does_not_change_results(eng, mode, W, P, win, cap):
    """Test 6: max_batch = 1, 3 and 64 -- a group cut short continues in the next one with later chunks."""
    signals = _signals(61)
    res = []
    for max_batch in (1, 3, 64):
        r = _restorer(eng, mode, W, P, win, cap, max_batch=max_batch)
        slots = [r.open() for _ in signals]
        res.append(_play(r, signals, slots, _events(62, W, P, mode), mode, W, P))
        r.shutdown()
    for x, a, b, c in zip(signals, *res):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, _offline(eng, mode, W, P, win, x))


def test_refusals(eng):
    """Test 7."""
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.streaming import StreamRestorer
    with pytest.raises(ValueError, match="one of the two"):
        StreamRestorer(_toy_net, 64, hop_size=16, in_margin=8, engine=eng)
    with pytest.raises(ValueError, match="even"):
        StreamRestorer(_toy_net, 63, hop_size=16, engine=eng)
    with pytest.raises(RuntimeError, match="even"):
        eng.stream_create(2, _lib.STREAM_OLA, 63, 16, None, 0.25, 128, 128)
    with pytest.raises(RuntimeError, match="input ring"):
        eng.stream_create(2, _lib.STREAM_BOXCAR, 64, 8, None, 1.0, 79, 128)
    # an overrun push names the slot and copies nothing: the session's later output is unchanged
    W, H, cap = 64, 16, 100
    x = _signals(71, (300,))[0]
    r = _restorer(eng, sr.OLA, W, H, "hanning", cap, slots=2)
    a, b = r.open(), r.open()
    y = [r.feed({a: x[:90], b: x[:50]})[a]]
    room = eng.stream_room(r._st, b)
    assert room == cap - 50 + (50 // H + 1) * H - W
    junk = torch.full((room + 1 + 10,), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="overrun the input ring of slot %d" % b):
        eng.stream_push(r._st, [a, b], [10, room + 1], junk)
    assert r.state(a) == (90, sr.released_before_close(sr.OLA, W, H, 90)) and r.state(b)[0] == 50
    y.append(r.feed({a: x[90:]})[a])
    y.append(r.close(a))
    assert torch.equal(torch.cat(y), _offline(eng, sr.OLA, W, H, "hanning", x))
    with pytest.raises(RuntimeError, match="slot %d is not open" % a):
        r.feed({a: x[:1]})
    with pytest.raises(RuntimeError, match="slot %d is not open" % a):
        r.feed({a: x[:0]})
    with pytest.raises(RuntimeError, match="no group is outstanding"):
        eng.stream_put(r._st, torch.zeros(1, W, device="cuda"))
    yb = torch.cat([r.feed({b: x[50:]})[b], r.close(b)])
    assert torch.equal(yb, _offline(eng, sr.OLA, W, H, "hanning", x))
    r.shutdown()
    # a full output ring: nothing more is scheduled, and scheduling resumes after a pop
    st = eng.stream_create(1, _lib.STREAM_BOXCAR, 64, 0, None, 1.0, 256, 64)
    s = eng.stream_open(st)
    x = _signals(72, (200,))[0]
    chunks = torch.empty(8 * 64, device="cuda")
    eng.stream_push(st, [s], [200], x)
    want = _offline(eng, sr.BOXCAR, 64, 0, None, x[:192])
    for k in range(3):      # frames 0, 1, 2 are all due; one fills the output ring of 64
        assert eng.stream_next(st, 8, chunks) == (1, 64)
        assert torch.equal(chunks[:64], x[64 * k:64 * k + 64])
        eng.stream_put(st, _toy_net(chunks[:64].view(1, 1, 64))["wav"].reshape(1, 64).contiguous())
        assert eng.stream_next(st, 8, chunks) == (0, 0)
        assert eng.stream_available(st, s) == 64
        assert torch.equal(eng.stream_pop(st, [s], [64])[0], want[64 * k:64 * k + 64])
    assert eng.stream_next(st, 8, chunks) == (0, 0) and eng.stream_state(st, s) == (200, 192)
    eng.stream_destroy(st)


@pytest.fixture(scope="module")
def voicefixer(engine, unet_sd, voc_sd):
    from voicefixer_main_amd.models import VoiceFixer
    m = VoiceFixer(None, channels=2, type_target="vocals", engine=engine)
    sd = {"generator.analysis_module." + k: v for k, v in unet_sd.items()}
    sd.update({"vocoder.model." + k: v for k, v in voc_sd.items()})
    m.load_state_dict(sd)
    return m.eval().to(torch.device("cuda:0"))


def test_real_network_streams_equal_offline_boxcar(voicefixer):
    """Test 8: VoiceFixer.restore on synthetic weights (built as test_chunked_restore_batched_equals_sequential builds it), boxcar
    mode, W = 22050, M = 4410; two streams of 1.7 s and 2.6 s fed in 0.37-s blocks."""
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.chunker import LambdaOverlapAddBoxcar
    from voicefixer_main_amd.streaming import StreamRestorer
    nnet = lambda c: {"wav": voicefixer.restore(c)}   # noqa: E731
    W, M, blk = 22050, 4410, int(0.37 * 44100)
    signals = [torch.from_numpy(synth.make_clips(1, sec, seed=seed)).cuda()[0, 0] for sec, seed in ((1.7, 81), (2.6, 82))]
    r = StreamRestorer(nnet, W, in_margin=M, window=None, slots=2, engine=voicefixer.engine)
    slots = [r.open(), r.open()]
    events = [{j: min(blk, x.numel() - t) for j, x in enumerate(signals) if x.numel() > t} for t in range(0, signals[1].numel(), blk)]
    got = _play(r, signals, slots, events, sr.BOXCAR, W, M)
    r.shutdown()
    off = LambdaOverlapAddBoxcar(nnet, 1, W, M, window=None, engine=voicefixer.engine)
    for x, y in zip(signals, got):
        want = off(x[None, None])[0, 0]
        assert y.shape == want.shape and torch.isfinite(y).all()
        assert torch.equal(y, want)
