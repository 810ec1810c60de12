"""GPU: the device array effects (Engine.quantize, Engine.time_dropout, csrc/effects.hip) and the list forms of simulate built on
them -- the quantiser bit for bit the host mirror, the drop-out bit for bit outside its smoothed patches and inside a derived bound in
them, padding never read, every clip independent of its batch -- and the effect chain `array_effects_list`."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import clips as vclips, simulate  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
C = 4096           # kClipChunk (csrc/clip_batch.h): samples of a clip per workgroup of the element-wise passes
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1, 3000]
DTYPES = [np.float32, np.float64]
BINS = [0, 1, 2, 3, 8, 12, 16]


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


def _clips_of(lengths, dtype, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * rng.uniform(0.05, 1.5)).astype(dtype) for n in lengths]


def _quant_host(clip, bins):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (0 / 0 of a silent clip)
        return simulate.quantification(clip, [True, bins])


def _assert_quant_equals_host(eng, clips, bins):
    """quantification_list of the clips as ONE call == the host mirror clip by clip, bit for bit"""
    got = simulate.quantification_list(clips, bins, engine=eng)
    assert len(got) == len(clips)
    for i, (g, c, b) in enumerate(zip(got, clips, bins)):
        want = _quant_host(c, b)
        assert g.dtype == want.dtype == np.float64 and g.shape == c.shape
        assert np.array_equal(g, want, equal_nan=True), "clip %d (%d samples, %d bins): %d differ" % (i, len(c), b, (g != want).sum())
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantiser_bit_for_bit(eng, dtype):
    clips = _clips_of(LENGTHS * 2, dtype, seed=1)
    bins = [BINS[i % len(BINS)] for i in range(len(clips))]
    assert set(bins) == set(BINS)
    got = _assert_quant_equals_host(eng, clips, bins)
    assert all(len(np.unique(g)) <= 2 ** b for g, b in zip(got, bins))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bins", [4, 16])
def test_level_boundaries(eng, dtype, bins):
    """peak exactly 1.0: +-1.0, every level, and its neighbours up and down in the clip's dtype"""
    level = 2 ** bins
    L = (-1 + (2 * np.arange(level) + 1) / level)
    assert np.array_equal(L.astype(dtype).astype(np.float64), L)      # (the levels are exact in float32 too)
    Lt = L.astype(dtype)
    clip = np.concatenate([np.array([-1.0, 1.0], dtype=dtype), Lt, np.nextafter(Lt, dtype(2)), np.nextafter(Lt, dtype(-2))])
    got, = _assert_quant_equals_host(eng, [clip], [bins])
    minus_one, one, on, up, down = got[0], got[1], got[2:2 + level], got[2 + level:2 + 2 * level], got[2 + 2 * level:]
    assert minus_one == 1 - 1 / level                 # -1.0 -> index -1 -> the top level
    assert one == L[-1]
    assert np.array_equal(on[1:], L[:-1])             # L_j -> L_{j-1}: the level strictly below
    assert on[0] == L[-1] == 1 - 1 / level            # L_0 -> L_{level-1}: the wrap again
    assert np.array_equal(up, L)                      # just above a level: that level
    assert np.array_equal(down[1:], L[:-1]) and down[0] == L[-1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_placement_of_the_peak(eng, dtype):
    rng = np.random.default_rng(2)
    clips, bins = [], []
    for n in (3000, C + 1):
        for pos, value in ((0, 0.9), (n - 1, 0.9), (1001, 0.9), (1001, -0.9), (0, -0.9), (n - 1, -0.9)):
            c = rng.uniform(-0.5, 0.5, n).astype(dtype)
            c[pos] = value
            clips.append(c)
            bins.append(BINS[len(clips) % len(BINS)])
    _assert_quant_equals_host(eng, clips, bins)
    x = vclips.pad(clips, DEV, torch.from_numpy(clips[0]).dtype)
    _, peaks = eng.quantize(x, bins, lengths=[len(c) for c in clips])
    assert peaks.dtype == x.dtype and np.array_equal(peaks.cpu().numpy(), np.full(len(clips), 0.9, dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_silent_clip_and_nan(eng, dtype):
    rng = np.random.default_rng(3)
    silent = np.zeros(C + 5, dtype=dtype)
    one_nan = rng.uniform(-0.5, 0.5, C + 5).astype(dtype)
    one_nan[C + 1] = np.nan
    plain = rng.uniform(-0.5, 0.5, 700).astype(dtype)
    got = _assert_quant_equals_host(eng, [silent, one_nan, plain, silent[:3]], [3, 8, 12, 0])
    assert not got[0].any() and not np.signbit(got[0]).any() and not got[3].any()
    assert np.isnan(got[1]).all()
    assert np.isfinite(got[2]).all() and got[2].any()


# ---------------------------------------------------------------------------------------------------------------- time drop-out
def _drop_host(clip, start, end):
    """simulate.time_dropout with the integer range given"""
    y = clip.copy()
    y[start:end] = 0
    y = simulate.smooth(y, smooth_center=start)
    return simulate.smooth(y, smooth_center=end)


def _patch_mask(n, start, end):
    m = np.zeros(n, dtype=bool)
    for c in (start, end):
        if c >= 50 and n - c >= 50:
            m[c - 50:c + 46] = True
    return m


def _assert_drop(got, want, clip, start, end, what):
    """inside the patches |device - mirror| <= 2^-24 |mirror| + 2^-45 max |clip| (the first term for float32 clips only: the one
    rounding to float32); everywhere else bit-equal to the mirror, which is the input or zero.
    Where the bound comes from: the device sums 25 products in double, off by at most 25 * 1.958 * 2^-53 max |knot| < 49 * 2^-53
    max |knot| (1.958 = the largest row sum of |M|); SciPy's own evaluation of the spline was measured at 6.4 * 2^-53 of the clip's
    peak (tests/test_array_effects_host.py repeats that measurement against this bar); 2^-45 = 256 * 2^-53 leaves about 4.5 x over
    their sum."""
    n = len(clip)
    assert got.dtype == want.dtype == clip.dtype and got.shape == clip.shape, what
    m = _patch_mask(n, start, end)
    bar = 2.0 ** -45 * float(np.abs(clip).max()) + (2.0 ** -24 * np.abs(want.astype(np.float64)) if clip.dtype == np.float32 else 0.0)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= bar)[m].all(), "%s: %g over the bar" % (what, (err - bar)[m].max())
    plain = clip.copy()
    plain[start:end] = 0
    assert np.array_equal(got[~m], want[~m]) and np.array_equal(got[~m], plain[~m]), what


DROP_CASES = [      # (n, start, end)
    (300, 49, 150), (300, 50, 150),            # the first centre 49 / 50 samples from the clip's start
    (300, 251, 260), (300, 250, 260),          # ... 49 / 50 from its end
    (300, 10, 49), (300, 10, 50),              # the second centre 49 / 50 from the start
    (300, 100, 251), (300, 100, 250),          # ... 49 / 50 from the end
    (300, 150, 150),                           # nothing zeroed, the same patch twice
    (400, 150, 151), (400, 150, 154), (400, 150, 196), (400, 150, 245), (400, 150, 246), (400, 150, 247), (400, 150, 250),
    (300, 200, 350), (300, 0, 300), (300, 299, 300), (99, 40, 60), (100, 50, 50), (1, 0, 1),
    (C + 200, C - 20, C + 30), (2 * C + 1, C - 50, 2 * C - 49), (3000, 1000, 1500),
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_time_dropout(eng, dtype):
    assert {e - s for n, s, e in DROP_CASES if n == 400} == {1, 4, 46, 95, 96, 97, 100}      # the second patch reads the first
    clips = _clips_of([n for n, _, _ in DROP_CASES], dtype, seed=4)
    order = sorted(range(len(clips)), key=lambda i: len(clips[i]))
    lens = [len(clips[i]) for i in order]
    x = vclips.pad([clips[i] for i in order], DEV, torch.from_numpy(clips[0]).dtype, width=(lens[-1] + 3) // 4 * 4)
    y = eng.time_dropout(x, [DROP_CASES[i][1] for i in order], [DROP_CASES[i][2] for i in order], lengths=lens)
    assert y.dtype == x.dtype and y.shape == x.shape
    y = y.cpu().numpy()
    patched = 0
    for row, i in enumerate(order):
        n, start, end = DROP_CASES[i]
        assert not y[row, n:].any()
        _assert_drop(y[row, :n], _drop_host(clips[i], start, end), clips[i], start, end, "case %s" % (DROP_CASES[i],))
        patched += _patch_mask(n, start, end).any()
    assert patched >= 18


@pytest.mark.parametrize("dtype", DTYPES)
def test_independence_and_padding(eng, dtype):
    """rows that hold NaN past each length, at a row stride that is no multiple of 4 (rows start off a 16-byte boundary): every clip
    bit-equal to its own single-clip call, rows zero past the length"""
    lengths = [3000, 1, 257, C + 1, 2999, 2 * C - 1, 66, C]
    L = 2 * C + 3
    clips = _clips_of(lengths, dtype, seed=5)
    x = np.full((len(lengths), L), np.nan, dtype=dtype)
    for b, c in enumerate(clips):
        x[b, :len(c)] = c
    xd = torch.from_numpy(x).to(DEV)
    bins = [BINS[b % len(BINS)] for b in range(len(lengths))]
    starts = [n // 3 for n in lengths]
    ends = [n // 3 + min(n // 2, 70 + 30 * b) for b, n in enumerate(lengths)]
    q, peaks = eng.quantize(xd, bins, lengths=lengths)
    d = eng.time_dropout(xd, starts, ends, lengths=lengths)
    assert q.shape == d.shape == (len(lengths), L) and q.dtype == torch.float64 and d.dtype == xd.dtype
    q, d, peaks = q.cpu().numpy(), d.cpu().numpy(), peaks.cpu().numpy()
    for b, c in enumerate(clips):
        n = len(c)
        assert not q[b, n:].any() and not d[b, n:].any() and np.isfinite(q[b, :n]).all() and np.isfinite(d[b, :n]).all()
        q1, p1 = eng.quantize(torch.from_numpy(c).to(DEV), bins[b])
        d1 = eng.time_dropout(torch.from_numpy(c).to(DEV), starts[b], ends[b])
        assert q1.shape == d1.shape == (n,) and p1.dim() == 0
        assert np.array_equal(q[b, :n], q1.cpu().numpy()) and peaks[b] == p1.item() == np.abs(c).max()
        assert np.array_equal(d[b, :n], d1.cpu().numpy())
        assert np.array_equal(q[b, :n], _quant_host(c, bins[b]))
        _assert_drop(d[b, :n], _drop_host(c, starts[b], ends[b]), c, starts[b], ends[b], "row %d" % b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_clips_than_one_launch_set(eng, dtype):
    """130 clips in one Engine call: the lengths, bins and ranges of 128 clips travel per set of launches (kFxMaxClips)"""
    lengths = [5 + 3 * b for b in range(130)]
    clips = _clips_of(lengths, dtype, seed=7)
    x = vclips.pad(clips, DEV, torch.from_numpy(clips[0]).dtype)
    bins = [BINS[b % len(BINS)] for b in range(130)]
    starts, ends = [n // 4 for n in lengths], [n // 2 for n in lengths]
    q, peaks = eng.quantize(x, bins, lengths=lengths)
    d = eng.time_dropout(x, starts, ends, lengths=lengths)
    q, peaks, d = q.cpu().numpy(), peaks.cpu().numpy(), d.cpu().numpy()
    for b, c in enumerate(clips):
        n = len(c)
        assert np.array_equal(q[b, :n], _quant_host(c, bins[b])) and not q[b, n:].any() and peaks[b] == np.abs(c).max(), "row %d" % b
        _assert_drop(d[b, :n], _drop_host(c, starts[b], ends[b]), c, starts[b], ends[b], "row %d" % b)
        assert not d[b, n:].any()


# ---------------------------------------------------------------------------------------------------------------- the chain
def test_chain(eng):
    rng = np.random.default_rng(6)
    F32 = np.float32
    n_of = [3000, C + 1, 700, 64, 2 * C + 1, 999, 3000, C, 2500, 1200, 800, C - 1]
    clips = [(rng.standard_normal(n) * rng.uniform(0.05, 0.9)).astype(F32) for n in n_of]
    clips[1] = (clips[1] * 20000).astype(F32)       # LARGESCALE
    clips[11] = (clips[11] * 20000).astype(F32)
    clips[5] = clips[5].astype(np.float64)
    rirs = [np.array([1.0, 0.0, 0.5, -0.25], dtype=F32), (rng.standard_normal(300) * 0.1).astype(F32)]
    drop = lambda s, t: [True, [s, t]]      # noqa: E731
    none = [True, None]
    dicts = [
        {"quant": [[True], 8]},
        {"quant": [[True], 3]},
        {"empty_c": none},
        {"quant": [[True], 4], "empty_c": none},
        {"time_dropout": drop(0.3, 0.1)},
        {"time_dropout": drop(0.5, 0.02), "beep": none},
        {"reverb_rir": [True, 1], "time_dropout": drop(0.2, 0.15), "quant": [[True], 12]},
        {"quant": [[True], 2], "time_dropout": drop(0.6, 0.3)},
        {"time_dropout": drop(0.1, 0.05), "reverb_rir": [True, 0]},
        {"reverb_rir": [True, 1], "quant": [[True], 16]},
        {"quant": [[True], 5], "empty_n": none, "reverb_rir": [True, 0]},
        {"time_dropout": drop(0.4, 0.2), "quant": [[True], 6]},
    ]
    keep = [c.copy() for c in clips]
    got = simulate.array_effects_list(clips, dicts, rirs, engine=eng)
    assert len(got) == 12 and all(np.array_equal(c, k) for c, k in zip(clips, keep))
    on_device = simulate.array_effects_list(clips, dicts, rirs, engine=eng, to_host=False)
    for i, (g, c, d) in enumerate(zip(got, clips, dicts)):
        steps = [k for k in d if k in ("reverb_rir", "time_dropout", "quant")]
        # the composition of the three device list forms, by hand
        if "empty_c" in d:
            want = np.zeros_like(c)
        else:
            large = c.max() > 10
            cur = torch.from_numpy(c).to(DEV)
            cur = cur / 2 ** 15 if large else cur
            for k in steps:
                if k == "reverb_rir":
                    cur, = simulate.reverb_rir_list([cur], rirs, rir_index=[d[k][1]], engine=eng, to_host=False)
                elif k == "time_dropout":
                    cur, = simulate.time_dropout_list([cur], d[k], engine=eng, to_host=False)
                else:
                    cur, = simulate.quantification_list([cur], d[k][1], engine=eng, to_host=False)
            want = (cur * 2 ** 15 if large else cur).cpu().numpy()
        assert isinstance(g, np.ndarray) and g.dtype == want.dtype and np.array_equal(g, want), "item %d" % i
        assert on_device[i].device == DEV and np.array_equal(on_device[i].cpu().numpy(), g)
        assert g.dtype == (np.float64 if "quant" in steps or c.dtype == np.float64 else F32) or "empty_c" in d
        # ... and the host: bit for bit where only the quantiser (or nothing) ran, inside the bar for the drop-out alone.  Chains
        # through the device reverb are not compared: its rounding differs within its own bound, and a quantiser behind it may
        # then pick a neighbouring level.
        if steps in (["quant"], []) or "empty_c" in d:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                host = simulate.array_effects(c, d, rirs)
            assert host.dtype == g.dtype and np.array_equal(g, host), "item %d" % i
        elif steps == ["time_dropout"]:
            start, end = simulate._dropout_range(len(c), d["time_dropout"])
            _assert_drop(g, simulate.array_effects(c, d, rirs), c, start, end, "item %d" % i)
    assert clips[1].max() > 10 and np.abs(got[1]).max() > 10 and not got[2].any() and not got[3].any()


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_refusals(eng, dtype):
    x = torch.rand((2, 400), device=DEV, dtype=dtype) - 0.5
    yq = torch.full((2, 400), 7.0, device=DEV, dtype=torch.float64)
    yd = torch.full((2, 400), 7.0, device=DEV, dtype=dtype)
    with pytest.raises(RuntimeError, match="bins"):
        eng.quantize(x, [3, 17], _y=yq)
    with pytest.raises(RuntimeError, match="bins"):
        eng.quantize(x, [-1, 3], _y=yq)
    with pytest.raises(RuntimeError, match="empty"):
        eng.quantize(x, 3, lengths=[400, 0], _y=yq)
    with pytest.raises(RuntimeError, match="401 samples"):
        eng.quantize(x, 3, lengths=[401, 400], _y=yq)
    with pytest.raises(RuntimeError, match="need 0 <= start <= end"):
        eng.time_dropout(x, [10, 200], [100, 199], _y=yd)
    with pytest.raises(RuntimeError, match="need 0 <= start <= end"):
        eng.time_dropout(x, [-1, 200], [100, 300], _y=yd)
    with pytest.raises(RuntimeError, match="empty"):
        eng.time_dropout(x, 10, 100, lengths=[0, 400], _y=yd)
    with pytest.raises(ValueError):
        eng.quantize(x.to(torch.float16), 3)
    with pytest.raises(ValueError):
        eng.time_dropout(x, [1, 2, 3], [4, 5, 6])
    # the C entry points with a row stride of y that does not hold the clips, a negative one included
    import ctypes
    from voicefixer_main_amd.simulate import smooth_matrix
    f64, lens, ptr = int(dtype == torch.float64), (ctypes.c_int64 * 2)(400, 400), lambda t: ctypes.c_void_p(t.data_ptr())
    for ldy in (399, -1):
        assert eng.lib.vfx_quantize(eng.h, ptr(x), f64, 2, 400, lens, (ctypes.c_int * 2)(3, 3), ptr(yq), ldy, None, None) != 0
        assert b"the rows hold 400 and %d" % ldy in eng.lib.vfx_last_error()
        assert eng.lib.vfx_time_dropout(eng.h, ptr(x), f64, 2, 400, lens, (ctypes.c_int64 * 2)(10, 10), (ctypes.c_int64 * 2)(100, 100),
                                        smooth_matrix().ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ptr(yd), ldy, None) != 0
        assert b"the rows hold 400 and %d" % ldy in eng.lib.vfx_last_error()
    torch.cuda.synchronize()
    assert (yq == 7.0).all() and (yd == 7.0).all()      # nothing was launched
    q, _ = eng.quantize(x, [3, 16], _y=yq)              # ... and the same buffers take the good calls
    d = eng.time_dropout(x, [10, 200], [100, 200], _y=yd)
    assert q.data_ptr() == yq.data_ptr() and d.data_ptr() == yd.data_ptr()
    assert not (yq == 7.0).any() and not (yd == 7.0).any()
