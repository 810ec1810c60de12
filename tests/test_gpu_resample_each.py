"""GPU: the per-clip resampler (Engine.resample_each, csrc/resample.hip k_resample_each) against scipy.signal.resample_poly bit for
bit in float32 and float64, its taps cache and errors, and the simulator's "stft" paths on the real engine."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

import resample_each_ref as ref

pytestmark = pytest.mark.gpu

FS = 44100
DEV = torch.device("cuda:0")
BLOCK = 256      # kResampleEachBlock: the outputs one workgroup owns
RATES = (7554, 2468, 22048, 21998, 29, 2000)      # each against 44100, both ways; 29 is c = 15: M = 44100, the largest filter
PAIRS = [p for r in RATES for p in ((FS, r), (r, FS))] + [(1, 2), (2, 1), (3, 7), (7, 3)]
LONG = (7554, 29)      # the pairs that also run a 3-s clip (132 300 samples at 44.1 kHz)


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need an MI355X (run with -m 'not gpu' elsewhere)")
    e = Engine("cuda:0")
    yield e
    e.close()


def _scipy(x, sr_in, sr_out):
    up, down = ref.reduced(sr_out, sr_in)
    return resample_poly(x, up, down)


def _signals(rng, n, dtype):
    """a random signal and a full-scale one (every sample at -1 or at the largest PCM16 value), as tests/test_gpu_resample.py"""
    return (rng.uniform(-1, 1, n).astype(dtype), np.where(rng.random(n) < 0.5, -1.0, 32767 / 32768).astype(dtype))


def _lengths(sr_in, sr_out):
    """1 and 2; a clip that lies inside the filter's half length (fewer than hl / up samples); the input lengths whose output lengths
    come nearest to one block's run of outputs - 1, exactly, + 1 and twice that; 3 s for the LONG pairs."""
    up, down = ref.reduced(sr_out, sr_in)
    hl = 10 * max(up, down)
    ns = [1, 2, max(3, hl // up // 2)]
    assert ns[2] < hl / up
    for target in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK):
        n = max(1, target * down // up)
        ns.append(min((n, n + 1), key=lambda v: abs(ref.out_len(v, up, down) - target)))
    if sr_in == FS and sr_out in LONG:
        ns.append(3 * FS)
    if sr_out == FS and sr_in in LONG:
        ns.append(ref.out_len(3 * FS, sr_in, FS))
    return sorted(set(ns))


def _pad(clips, dtype, fill=0.0):
    x = torch.full((len(clips), max(len(c) for c in clips)), fill, dtype=dtype)
    for b, c in enumerate(clips):
        x[b, :len(c)] = torch.from_numpy(c)
    return x.to(DEV)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_every_pair_is_resample_poly_bit_for_bit(eng, sr_in, sr_out, dtype):
    """All lengths and both signals of a pair as ONE padded batch (rows past a clip's length hold a sentinel the kernel must not read),
    and the first clips again as 1-D calls."""
    rng = np.random.default_rng(sr_in * 7 + sr_out)
    clips = [x for n in _lengths(sr_in, sr_out) for x in _signals(rng, n, dtype)]
    want = [_scipy(x, sr_in, sr_out) for x in clips]
    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    y, out_lengths = eng.resample_each(_pad(clips, tdtype, fill=1e30), sr_in, sr_out, lengths=[len(c) for c in clips])
    assert y.dtype == tdtype and y.shape == (len(clips), max(len(w) for w in want))
    assert out_lengths == [len(w) for w in want]
    y = y.cpu().numpy()
    for b, w in enumerate(want):
        assert w.dtype == dtype and np.array_equal(y[b, :len(w)], w), (sr_in, sr_out, len(clips[b]), np.abs(y[b, :len(w)] - w).max())
        assert not y[b, len(w):].any()
    for x, w in list(zip(clips, want))[:6]:
        y1, n1 = eng.resample_each(torch.from_numpy(x).to(DEV), sr_in, sr_out)
        assert n1 == len(w) and y1.dtype == tdtype and y1.shape == w.shape and np.array_equal(y1.cpu().numpy(), w)


MIXED = [(FS, 7554), (2468, FS), (FS, 29), (FS, 7554), (3, 7), (FS, FS), (22048, FS), (2468, FS), (FS, 29)]
MIXED_LENGTHS = (3000, 211, 70001, 1, 640, 777, 1500, 2, 44100)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_mixed_call(eng, dtype):
    """9 clips of unequal lengths (1 included), five distinct pairs -- three of them shared by two clips -- and one clip at the same
    rate: each row is its own single-clip call and SciPy's result, zero from its output length to n_out in a y handed in full of NaN,
    and a permuted call gives the permuted rows."""
    assert len(set(MIXED)) == 6 and len(set(MIXED) - {(FS, FS)}) == 5
    rng = np.random.default_rng(9)
    clips = [rng.uniform(-1, 1, n).astype(dtype) for n in MIXED_LENGTHS]
    want = [_scipy(x, i, o) for x, (i, o) in zip(clips, MIXED)]
    assert np.array_equal(want[5], clips[5])
    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    n_out = max(len(w) for w in want) + 37
    lens = [len(c) for c in clips]

    def run(order):
        y = torch.full((9, n_out), float("nan"), dtype=tdtype, device=DEV)
        got, out_lengths = eng.resample_each(_pad([clips[i] for i in order], tdtype), [MIXED[i][0] for i in order], [MIXED[i][1] for i in order],
                                             lengths=[lens[i] for i in order], n_out=n_out, _y=y)
        assert got.data_ptr() == y.data_ptr() and out_lengths == [len(want[i]) for i in order]
        return got.cpu().numpy()

    y = run(range(9))
    for b, w in enumerate(want):
        assert np.array_equal(y[b, :len(w)], w), (b, MIXED[b])
        assert np.array_equal(y[b, len(w):], np.zeros(n_out - len(w), dtype))
        y1, n1 = eng.resample_each(torch.from_numpy(clips[b]).to(DEV), *MIXED[b])
        assert n1 == len(w) and np.array_equal(y1.cpu().numpy(), w)
    order = [int(i) for i in np.random.default_rng(1).permutation(9)]
    assert np.array_equal(run(order), y[order])
    # n_out below the longest output cuts the rows
    cut, _ = eng.resample_each(_pad(clips, tdtype), [p[0] for p in MIXED], [p[1] for p in MIXED], lengths=lens, n_out=300)
    assert cut.shape == (9, 300) and np.array_equal(cut.cpu().numpy(), y[:, :300])


def test_130_clips_are_cut_into_calls_of_128(eng):
    rng = np.random.default_rng(130)
    pairs = [((FS, 2000), (3, 7), (2, 1))[b % 3] for b in range(130)]
    clips = [rng.uniform(-1, 1, int(n)).astype(np.float32) for n in rng.integers(50, 181, 130)]
    y, out_lengths = eng.resample_each(_pad(clips, torch.float32), [p[0] for p in pairs], [p[1] for p in pairs], lengths=[len(c) for c in clips])
    y = y.cpu().numpy()
    for b, (x, (i, o)) in enumerate(zip(clips, pairs)):
        w = _scipy(x, i, o)
        assert out_lengths[b] == len(w) and np.array_equal(y[b, :len(w)], w) and not y[b, len(w):].any(), b


def test_taps_cache_evicts_least_recently_used(eng, monkeypatch):
    """A budget of two designs (M = 441 and M = 147, float32): a call that needs three keeps all three, a later call evicts them
    oldest first until the budget holds, and the first call repeated after that is right again."""
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, (3, 500)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    f32 = torch.float32
    eng._resample_each_cache.clear()
    monkeypatch.setattr(eng, "RESAMPLE_EACH_CACHE_BYTES", 4 * (20 * 441 + 1 + 20 * 147 + 1))

    def check(sr_in, sr_out):
        y, lens = eng.resample_each(xd, sr_in, sr_out)
        for b in range(3):
            w = _scipy(x[b], sr_in[b], sr_out[b])
            assert lens[b] == len(w) and np.array_equal(y[b, :len(w)].cpu().numpy(), w)

    first = ([FS] * 3, [2000] * 3)
    check(*first)
    assert list(eng._resample_each_cache) == [(441, f32)]
    check([FS, FS, 3], [2000, 300, 7])      # M = 441, 147, 7: past the budget, all needed
    assert set(eng._resample_each_cache) == {(441, f32), (147, f32), (7, f32)}
    check([FS] * 3, [147] * 3)              # M = 300: the three of the call before go, oldest first, until M = 300 fits with the rest
    assert list(eng._resample_each_cache) == [(300, f32)]
    check(*first)
    assert list(eng._resample_each_cache) == [(441, f32)]
    total = sum(t.numel() * t.element_size() for t in eng._resample_each_cache.values())
    assert total <= eng.RESAMPLE_EACH_CACHE_BYTES


def test_errors_launch_nothing(eng):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, 400)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    y = torch.full((2, 50), 5.0, dtype=torch.float32, device=DEV)

    def valid():
        got, _ = eng.resample_each(xd, FS, [2000, 7554], n_out=50, _y=y)
        for b, r in enumerate((2000, 7554)):
            assert np.array_equal(got[b].cpu().numpy(), np.pad(_scipy(x[b], FS, r), (0, 50))[:50])
        y.fill_(5.0)

    with pytest.raises(RuntimeError, match=r"clip 1: 65536 Hz -> 65537 Hz is the pair 65537/65536"):
        eng.resample_each(xd, [FS, 65536], [2000, 65537], n_out=50, _y=y)
    assert bool((y == 5.0).all())
    valid()
    with pytest.raises(TypeError, match="float32 or float64"):
        eng.resample_each(torch.zeros((2, 400), dtype=torch.int16, device=DEV), FS, 2000, n_out=50, _y=y)
    assert bool((y == 5.0).all())
    valid()
    # the C entry point itself: an error through vfx_last_error, y untouched
    taps, at = eng._resample_each_taps([441], torch.float32)

    def call(index, up=(20, 1), down=(441, 1), lengths=(400, 400), B=2, F=2):
        return eng.lib.vfx_resample_each(eng.h, ctypes.c_void_p(xd.data_ptr()), 0, B, 400, (ctypes.c_int64 * 2)(*lengths),
                                         (ctypes.c_int * 2)(*index), (ctypes.c_int * 2)(*up), (ctypes.c_int * 2)(*down),
                                         ctypes.c_void_p(taps.data_ptr()), (ctypes.c_int64 * 2)(at[441], 0), F,
                                         ctypes.c_void_p(y.data_ptr()), 50, 50, None)

    assert call([0, 2]) != 0 and b"clip 1 asks for design 2 of 2" in eng.lib.vfx_last_error()
    assert call([-1, 0]) != 0 and b"clip 0 asks for design -1 of 2" in eng.lib.vfx_last_error()
    assert call([0, 1], up=(20, 2 * 65537), down=(441, 2 * 65536)) != 0
    assert b"clip 1" in eng.lib.vfx_last_error() and b"65537/65536" in eng.lib.vfx_last_error()
    assert call([0, 1], lengths=(400, -1)) != 0 and b"clip 1 has a negative length" in eng.lib.vfx_last_error()
    assert call([0, 1], lengths=(401, 400)) != 0
    assert call([0, 1], up=(0, 1)) != 0
    assert call([0, 1], B=0) != 0 and call([0, 1], B=129) != 0 and call([0, 1], F=0) != 0 and call([0, 1], F=129) != 0
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())
    assert call([0, 1]) == 0      # design 1 is the same rate: a copy
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.array_equal(got[0], np.pad(_scipy(x[0], FS, 2000), (0, 50))[:50]) and np.array_equal(got[1], x[1, :50])
    y.fill_(5.0)
    valid()


def test_natural_tap_order_gives_the_same_bits(eng):
    """the handle's debug switch (the taps in natural order instead of phase-major) changes no bit"""
    from voicefixer_main_amd import _lib
    tlib = _lib.load_test()
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.uniform(-1, 1, (4, 3000))).to(DEV)
    rates = [7554, 29, 2468, 21998]
    want_down, lens = eng.resample_each(x, FS, rates)
    want_up, _ = eng.resample_each(want_down, rates, FS, lengths=lens)
    assert tlib.vfx_debug_resample_each_layout(eng.h, 1) == 0
    try:
        down, _ = eng.resample_each(x, FS, rates)
        up, _ = eng.resample_each(down, rates, FS, lengths=lens)
    finally:
        assert tlib.vfx_debug_resample_each_layout(eng.h, 0) == 0
    assert torch.equal(down, want_down) and torch.equal(up, want_up)
    for b, r in enumerate(rates):
        assert np.array_equal(want_down[b, :lens[b]].cpu().numpy(), _scipy(x[b].cpu().numpy(), FS, r))


# ------------------------------------------------------------------------------------------------------------ the simulator
@pytest.fixture
def counted(eng, monkeypatch):
    """simulate.stft_hard_lowpass raises and Engine.resample_each counts: -> the list of (dtype, clips, n_out) per call.  A test
    computes what it compares with BEFORE asking for this."""
    from voicefixer_main_amd import simulate
    from voicefixer_main_amd.engine import Engine
    calls = []
    inner = Engine.resample_each

    def counting(self, x, sr_in, sr_out, lengths=None, n_out=None, **kw):
        calls.append((x.dtype, x.shape[0], n_out))
        return inner(self, x, sr_in, sr_out, lengths=lengths, n_out=n_out, **kw)

    def host(*a, **kw):
        raise AssertionError("an item took the host function")

    monkeypatch.setattr(Engine, "resample_each", counting)
    monkeypatch.setattr(simulate, "stft_hard_lowpass", host)
    return calls


def _pairs_of_calls(calls):
    """the calls as (down, up) pairs: one dtype and clip count per pair, down with n_out left alone -> [(dtype, clips)]"""
    assert len(calls) % 2 == 0
    for d, u in zip(calls[::2], calls[1::2]):
        assert d[:2] == u[:2] and d[2] is None and u[2] is not None
    return [c[:2] for c in calls[::2]]


def test_lowpass_list_and_each_on_the_engine(eng, request):
    from voicefixer_main_amd import simulate
    rng = np.random.default_rng(12)
    clips = [rng.uniform(-1, 1, n).astype(np.float64 if i in (1, 4) else np.float32) for i, n in enumerate((1500, 2999, 1000, 2200, 1001, 1777))]
    cuts = [1234, 3777, 15, 11024, 22049, 750]
    want_list = {c: [simulate.lowpass(x, c, FS, _type="stft") for x in clips] for c in (1234, 3777)}
    want_each = [simulate.lowpass(x, c, FS, _type="stft") for x, c in zip(clips, cuts)]
    calls = request.getfixturevalue("counted")
    f32, f64 = torch.float32, torch.float64
    for c, want in want_list.items():
        del calls[:]
        got = simulate.lowpass_list(clips, c, FS, _type="stft", engine=eng)
        dev = simulate.lowpass_list(clips, c, FS, _type="stft", engine=eng, to_host=False)
        assert _pairs_of_calls(calls) == [(f32, 4), (f64, 2)] * 2
        for i, (w, g, d) in enumerate(zip(want, got, dev)):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w), (c, i)
            assert d.device.type == "cuda" and d.cpu().numpy().dtype == w.dtype and np.array_equal(d.cpu().numpy(), w), (c, i)
    del calls[:]
    got = simulate.lowpass_each(clips, cuts, FS, types="stft", engine=eng)
    assert _pairs_of_calls(calls) == [(f32, 4), (f64, 2)]      # two calls per batch whatever its cut-offs
    for i, (w, g) in enumerate(zip(want_each, got)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (i, cuts[i])


def test_lowpass_collate_keeps_every_item_on_the_device(eng, request):
    """The seeded batch of tests/test_gpu_sosfilt_bank.py's collator test, 6 items of 4096 samples with all six types, against the
    loop over the single-clip functions -- then again with the host function forbidden: the "stft" follow-ups run on the float64
    device rows of the IIR pass."""
    from voicefixer_main_amd import simulate
    L, lo, hi, o_lo, o_hi = 4096, 1500, 44100, 2, 10
    types = ["cheby1", "ellip", "bessel", "stft_hard", "stft", "butter"]
    data = np.random.default_rng(6)
    batch = [{"fname": "item%d" % i, "vocals": data.uniform(-1, 1, (L, 1)).astype(np.float32),
              "noise": data.uniform(-1, 1, (L, 1)).astype(np.float32)} for i in range(6)]
    rng = np.random.default_rng(66)

    def uniform(lower, upper):
        return (upper - lower) * rng.random() + lower

    def lowpass(x, c, o, f):
        return simulate.lowpass(x, highcut=c, fs=FS, order=o, _type=f, engine=eng)

    cutoffs, orders, filters = [], [], []
    for _ in batch:
        cutoffs.append(int(uniform(lo // 2, hi // 2)))
        orders.append(int(uniform(o_lo, o_hi)))
        filters.append(types[int(uniform(0, len(types)))])
    want, expect_pairs = {}, []
    for key in ("vocals", "noise"):
        want[key], first, again = [], [], []
        for x, c, o, f in zip(batch, cutoffs, orders, filters):
            chance = int(uniform(0, 1000))
            if key == "noise" and chance % 2 == 0:
                want[key].append(x[key][..., 0])
                continue
            if f == "stft":
                first.append(x[key].dtype)
            y = lowpass(x[key][..., 0], c, o, f)
            if chance % (2 if key == "vocals" else 3) == 0:
                again.append(y.dtype)
                y = lowpass(y, c, o, "stft")
            want[key].append(y)
        for dtypes in (first, again):      # a lowpass_each call: one batch per dtype that has "stft" items
            for name, t in (("float32", torch.float32), ("float64", torch.float64)):
                n = sum(1 for d in dtypes if str(d) == name)
                if n:
                    expect_pairs.append((t, n))
    assert any(t == torch.float64 for t, _ in expect_pairs)      # the draws do include a follow-up behind an IIR filter

    calls = request.getfixturevalue("counted")
    got = simulate.lowpass_collate(batch, [lo, hi], [o_lo, o_hi], types, FS, rng=np.random.default_rng(66), engine=eng)
    assert _pairs_of_calls(calls) == expect_pairs
    for key, rows in want.items():
        lr = got[key + "_LR"]
        assert lr.device.type == "cuda" and lr.dtype == torch.float32 and lr.shape == (6, L, 1)
        for i, w in enumerate(rows):
            assert np.array_equal(lr[i, :, 0].cpu().numpy(), w.astype(np.float32)), (key, i, filters[i], cutoffs[i], orders[i])


def test_lowpass_collate_val_on_the_engine(eng, request):
    from voicefixer_main_amd import simulate
    L = 3000
    rng = np.random.default_rng(8)
    batch = [{"fname": "v%d" % i, "vocals": rng.uniform(-1, 1, (L, 1)).astype(np.float32)} for i in range(3)]
    want = {c: [simulate.lowpass(simulate.lowpass(x["vocals"][..., 0], c, 44100, 8, "butter"), c, 44100, 8, "stft") for x in batch]
            for c in simulate.VAL_CUTOFFS}
    calls = request.getfixturevalue("counted")
    got = simulate.lowpass_collate_val(batch, engine=eng)
    assert _pairs_of_calls(calls) == [(torch.float64, 3)] * 5
    for c, rows in want.items():
        lr = got["vocalsLR_%d" % c]
        assert lr.device.type == "cuda" and lr.dtype == torch.float32 and lr.shape == (3, L, 1)
        for i, w in enumerate(rows):
            assert np.array_equal(lr[i, :, 0].cpu().numpy(), w.astype(np.float32)), (c, i)
