"""Host side of the array effects: the mirrors of MagicalEffects.quantification / time_dropout / smooth against the reference's own
outputs (tests/golden/array_effects.npz, scripts/gen_golden_array_effects.py), the matrix form of `smooth` that the device kernel
evaluates, the bindings of vfx_quantize and vfx_time_dropout, the list forms on items that take the host path, `array_effects` and
`draw_array_effects`.  No GPU, no Engine."""
import ctypes
import os
import re
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, simulate  # noqa: E402

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "array_effects.npz"))
DTYPES = [np.float32, np.float64]


def patch_bound(want, clip):
    """The bar inside a smoothed patch: 2^-24 |want| for the rounding to float32 (float32 clips only) + 2^-45 max |clip| for the
    float64 evaluation of the spline -- the 25-term sum is off by at most 25 * 1.958 * 2^-53 max |knot| < 49 * 2^-53, SciPy's own
    evaluation was measured at 6.4 * 2^-53, and 2^-45 = 256 * 2^-53 leaves about 4.5 x over their sum."""
    rel = 2.0 ** -24 * np.abs(want.astype(np.float64)) if want.dtype == np.float32 else 0.0
    return rel + 2.0 ** -45 * float(np.max(np.abs(clip)))


def patch_mask(n, start, end):
    """True where time_dropout's two smooth() calls write"""
    m = np.zeros(n, dtype=bool)
    for c in (start, end):
        if c >= 50 and n - c >= 50:
            m[c - 50:c + 46] = True
    return m


def assert_dropout(got, want, clip, start, end, what=""):
    """got against want (both time_dropout of clip): inside the bar in the patches; bit-equal, and the input or zero, elsewhere"""
    n = len(clip)
    assert got.dtype == want.dtype == clip.dtype and got.shape == want.shape == clip.shape, what
    m = patch_mask(n, start, end)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= patch_bound(want, clip))[m].all(), "%s: %g over the bar" % (what, (err - patch_bound(want, clip))[m].max())
    plain = clip.copy()
    plain[start:end] = 0
    assert np.array_equal(got[~m], want[~m]) and np.array_equal(got[~m], plain[~m]), what


def _golden_clips():
    for dtype in DTYPES:
        name = np.dtype(dtype).name
        for k in range(len(GOLDEN["lengths"])):
            yield name, k, GOLDEN["clip_%s_%d" % (name, k)]


def test_fixture_is_what_it_claims():
    clips = list(_golden_clips())
    assert len(clips) == 6 and {c.dtype for _, _, c in clips} == {np.dtype(d) for d in DTYPES}
    assert all(400 <= len(c) <= 3000 for _, _, c in clips)
    n = 400      # the shortest clip sees every case: overlapping patches, both skip conditions, a stretch past the end
    ranges = [simulate._dropout_range(n, [True, list(p)]) for p in GOLDEN["drop_params"]]
    assert any(0 < e - s < 96 and patch_mask(n, s, e).sum() < 192 and s >= 50 and n - e >= 50 for s, e in ranges)
    assert any(s < 50 <= e <= n - 50 for s, e in ranges) and any(s >= 50 and n - 50 < e <= n for s, e in ranges)
    assert any(e > n for s, e in ranges) and any(s == e for s, e in ranges)


def test_quantification_equals_the_reference_bit_for_bit():
    for name, k, clip in _golden_clips():
        for bins in GOLDEN["bins"]:
            want = GOLDEN["quant_%s_%d_b%d" % (name, k, bins)]
            got = simulate.quantification(clip.copy(), [True, int(bins)])
            assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want), (name, k, bins)
            assert len(np.unique(got)) <= 2 ** bins


def test_time_dropout_equals_the_reference():
    for name, k, clip in _golden_clips():
        for j, p in enumerate(GOLDEN["drop_params"]):
            params = [True, [float(p[0]), float(p[1])]]
            work = clip.copy()
            got = simulate.time_dropout(work, params)
            assert got is work      # in place, as the reference
            start, end = simulate._dropout_range(len(clip), params)
            assert_dropout(got, GOLDEN["drop_%s_%d_p%d" % (name, k, j)], clip, start, end, "%s %d p%d" % (name, k, j))


@pytest.mark.parametrize("dtype", DTYPES)
def test_smooth_matrix_against_smooth(dtype):
    """the matrix form the kernel evaluates, in NumPy, against the SciPy path: the reference itself stays inside the GPU test's bar"""
    M = simulate.smooth_matrix()
    assert M.shape == (96, 25) and M.dtype == np.float64 and not M.flags.writeable and simulate.smooth_matrix() is M
    assert np.abs(M).sum(axis=1).max() < 1.96
    assert np.abs(M[::4] - np.eye(25)[:24]).max() < 2.0 ** -50      # an interpolation: the knots themselves come back
    rng = np.random.default_rng(1952)
    for it in range(200):
        n = int(rng.integers(100, 700))
        c = int(rng.integers(50, n - 49))
        clip = (rng.standard_normal(n) * rng.uniform(1e-3, 30)).astype(dtype)
        if it % 2:      # a zeroed stretch beside the centre, as time_dropout leaves it
            clip[c:c + int(rng.integers(0, 120))] = 0
        want = simulate.smooth(clip.copy(), c)
        got = clip.copy()
        got[c - 50:c + 46] = (M @ clip[c - 50:c + 50:4].astype(np.float64)).astype(dtype)
        assert_dropout(got, want, clip, c, c, "clip %d" % it)
    short = rng.standard_normal(120).astype(dtype)
    for c in (49, 71):
        assert np.array_equal(simulate.smooth(short.copy(), c), short)
    two_d = rng.standard_normal((300, 1)).astype(dtype)
    y = simulate.smooth(two_d.copy(), 100)
    assert y.shape == (300, 1) and np.array_equal(y[:, 0], simulate.smooth(two_d[:, 0].copy(), 100))


def test_quantification_edges():
    level = 16
    L = -1 + (2 * np.arange(level) + 1) / level
    assert np.array_equal(L, np.linspace(-1 + 1 / level, 1 - 1 / level, level))
    # the wrap: the negative peak, and anything at or below the lowest level, comes out as the TOP level
    y = simulate.quantification(np.array([-1.0, L[0], 1.0, 0.0]), [True, 4])
    assert y[0] == y[1] == L[-1] == 1 - 1 / level
    assert y[2] == L[-1] and y[3] == L[7] == -1 / level
    # a sample exactly on a level goes to the level below it; just above it, to that level
    y = simulate.quantification(np.concatenate([[1.0], L[1:], np.nextafter(L, 2)]), [True, 4])
    assert np.array_equal(y[1:level], L[:-1]) and np.array_equal(y[level:], L)
    # the peak scales the levels; float32 in, float64 out
    y = simulate.quantification(np.array([0.5, -0.25, 0.1], dtype=np.float32), [True, 2])
    assert y.dtype == np.float64 and np.array_equal(y, np.array([0.75, -0.75, -0.25]) * 0.5)
    assert np.array_equal(simulate.quantification(np.array([0.3, -0.7]), [True, 0]), [0.0, 0.0])      # one level: 0
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        y = simulate.quantification(np.zeros(7, dtype=np.float32), [True, 3])
    assert np.array_equal(y, np.zeros(7)) and any("invalid value" in str(x.message) for x in w)
    y = simulate.quantification(np.array([0.5, np.nan, -1.0]), [True, 3])
    assert np.isnan(y).all()


@pytest.mark.parametrize("name, nargs", [("vfx_quantize", 11), ("vfx_time_dropout", 12)])
def test_signatures_match_the_header(name, nargs):
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
    res, args = _lib.SIGNATURES[name]
    vp, ip, lp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
    assert res is ctypes.c_int and len(decl.split(",")) == len(args) == nargs
    if name == "vfx_quantize":
        assert args == [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64, lp, ip, vp, ctypes.c_int64, vp, vp]
    else:
        assert args == [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64, lp, lp, lp, ctypes.POINTER(ctypes.c_double), vp,
                        ctypes.c_int64, vp]
    # the C types, argument by argument
    ctype = {vp: r"(const )?void\*|vfx_handle\*|double\*", ctypes.c_int: "int", ctypes.c_int64: "int64_t", ip: r"const int\*",
             lp: r"const int64_t\*", ctypes.POINTER(ctypes.c_double): r"const double\*"}
    for text, a in zip(decl.split(","), args):
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S).split()
        assert re.fullmatch(ctype[a], " ".join(text[:-1])), (text, a)


def _no_engine(monkeypatch):
    def boom():
        raise AssertionError("the host path must not create an Engine")
    monkeypatch.setattr(simulate, "_get_engine", boom)


def test_list_forms_on_the_host_path(monkeypatch):
    _no_engine(monkeypatch)
    rng = np.random.default_rng(4)
    f16 = (rng.standard_normal(300) * 0.3).astype(np.float16)
    i16 = (rng.standard_normal(400) * 3000).astype(np.int16)
    f32, f64 = (rng.standard_normal(500) * 0.5).astype(np.float32), rng.standard_normal(260) * 0.5
    two_d = rng.standard_normal((200, 1)).astype(np.float32)
    # quantiser: dtypes the device does not take, bins past its 16, a 2-D clip
    clips, bins = [f16, i16, f32, f64, two_d], [3, 8, 17, 17, 2]
    keep = [c.copy() for c in clips]
    got = simulate.quantification_list(clips, bins)
    for g, c, b in zip(got, clips, bins):
        want = simulate.quantification(c, [True, b])
        assert g.dtype == want.dtype and np.array_equal(g, want)
    assert len(np.unique(got[2])) > 400 and all(np.array_equal(c, k) for c, k in zip(clips, keep))
    one = simulate.quantification_list([f16, i16], 5)      # one bins for all
    assert np.array_equal(one[1], simulate.quantification(i16, [True, 5]))
    with pytest.raises(ValueError, match="2 entries for 3 clips"):
        simulate.quantification_list([f16, i16, f16], [1, 2])
    # drop-out: the same dtypes, and end < start on clips the device would take otherwise
    back = [True, [0.5, -0.1]]
    clips, params = [f16, i16, f32, f64], [[True, [0.3, 0.2]], [True, [0.2, 0.3]], back, back]
    keep = [c.copy() for c in clips]
    got = simulate.time_dropout_list(clips, params)
    for g, c, p in zip(got, clips, params):
        want = simulate.time_dropout(c.copy(), p)
        assert g.dtype == want.dtype == c.dtype and np.array_equal(g, want)
    assert all(np.array_equal(c, k) for c, k in zip(clips, keep))      # the inputs are never modified
    s, e = simulate._dropout_range(500, back)
    assert e < s and not np.array_equal(got[2], f32) and np.array_equal(got[2][:e - 50], f32[:e - 50])
    one = simulate.time_dropout_list([f16, i16], [True, [0.25, 0.5]])      # one params for all
    assert np.array_equal(one[0], simulate.time_dropout(f16.copy(), [True, [0.25, 0.5]])) and not one[0][125:175].any()
    with pytest.raises(ValueError, match="2 entries for 1 clips"):
        simulate.time_dropout_list([f16], [back, back])
    assert simulate.quantification_list([], 3) == [] and simulate.time_dropout_list([], back) == []


def test_array_effects(monkeypatch):
    _no_engine(monkeypatch)
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(1200) * 0.4).astype(np.float32)
    rirs = [np.array([1.0, 0.0, 0.5], dtype=np.float32), (rng.standard_normal(40) * 0.2).astype(np.float32)]
    drop, quant, rir = [True, [0.3, 0.1]], [[True], 4], [True, 1]
    keep = x.copy()
    # dict order is the order of application
    a = simulate.array_effects(x, {"time_dropout": drop, "quant": quant})
    b = simulate.array_effects(x, {"quant": quant, "time_dropout": drop})
    assert np.array_equal(a, simulate.quantification(simulate.time_dropout(x.copy(), drop), quant))
    assert np.array_equal(b, simulate.time_dropout(simulate.quantification(x, quant), drop)) and not np.array_equal(a, b)
    c = simulate.array_effects(x, {"quant": quant, "beep": [True, None], "reverb_rir": rir, "empty_n": [True, None]}, rirs)
    assert np.array_equal(c, simulate.reverb_rir(simulate.quantification(x, quant), rirs[1]))
    assert np.array_equal(simulate.array_effects(x, {}), x) and np.array_equal(x, keep)
    # empty_c wins wherever it stands, and returns before the rescale
    z = simulate.array_effects(x * 20000, {"quant": quant, "empty_c": [True, None]})
    assert z.dtype == np.float32 and z.shape == x.shape and not z.any()
    # LARGESCALE: / 2^15, the effects, * 2^15
    big = (x * 20000).astype(np.float32)
    got = simulate.array_effects(big, {"time_dropout": drop, "quant": quant})
    want = simulate.quantification(simulate.time_dropout(big / 2 ** 15, drop), quant) * 2 ** 15
    assert big.max() > 10 and np.array_equal(got, want)
    assert np.array_equal(simulate.array_effects(big, {}), big)      # the round trip alone is exact
    # the list form on clips that take the host path is the loop
    i16 = (x * 20000).astype(np.int16)
    dicts = [{"quant": quant}, {"empty_c": [True, None]}, {"time_dropout": drop, "quant": quant}]
    got = simulate.array_effects_list([i16, i16, x.astype(np.float16)], dicts)
    for g, c, d in zip(got, [i16, i16, x.astype(np.float16)], dicts):
        want = simulate.array_effects(c, d)
        assert g.dtype == want.dtype and np.array_equal(g, want)
    for fn, args in ((simulate.array_effects, (x,)), (simulate.array_effects_list, ([x],))):
        wrap = (lambda d: [d]) if fn is simulate.array_effects_list else (lambda d: d)
        for key in ("tempo", "fade", "low_pass", "anytime"):
            with pytest.raises(ValueError, match="sox chain, which is not built here"):
                fn(*args, wrap({"quant": quant, key: [True, 1.0]}))
        with pytest.raises(ValueError, match="Unknown effect"):
            fn(*args, wrap({"wobble": [True, None]}))
    with pytest.raises(ValueError, match="RIRs"):
        simulate.array_effects(x, {"reverb_rir": rir})
    with pytest.raises(ValueError, match="1 dicts for 2 clips"):
        simulate.array_effects_list([x, x], [{}])


P_EFFECTS = {
    "reverb_rir": {"prob": [0.8], "rir_file_name": None},
    "time_dropout": {"prob": [0.5], "max_segment": 0.2, "drop_range": [0.0, 1.0]},
    "quant": {"prob": [0.6, 0.3], "bins": [3, 12]},
    "empty_c": {"prob": [0.2]},
    "empty_n": {"prob": [1.0]},
    "beep": {"prob": [0.0]},
}


def test_draw_array_effects():
    names = ["quant", "beep", "time_dropout", "empty_n", "reverb_rir", "empty_c"]
    a, b = np.random.default_rng(31), np.random.default_rng(31)
    got = simulate.draw_array_effects(40, P_EFFECTS, names, 7, a)
    u = simulate._uniform
    for item in got:      # the hand-written loop: a chance per name, then the name's draws
        want = {}
        for name in names:
            chance = int(b.random() * 2 ** 31)
            dec = [chance < p * 2 ** 31 for p in P_EFFECTS[name]["prob"]]
            if not dec[0]:
                continue
            if name == "quant":
                want[name] = [dec, int(u(3, 12, b))]
            elif name == "time_dropout":
                start = u(0.0, 0.8, b)
                want[name] = [True, [start, u(0.0, 0.2, b)]]
            elif name == "reverb_rir":
                want[name] = [True, int(u(0, 7, b))]
            else:
                want[name] = [True, None]
        assert item == want and list(item) == list(want)      # ... in effect_list order
    assert a.random() == b.random()      # the generator is where the loop left it
    seen = {k for item in got for k in item}
    assert seen == set(names) - {"beep"} and all("empty_n" in item for item in got)
    assert all(3 <= item["quant"][1] < 12 and item["quant"][0][0] for item in got if "quant" in item)
    assert {tuple(item["quant"][0]) for item in got if "quant" in item} == {(True, True), (True, False)}
    assert all(0 <= item["reverb_rir"][1] < 7 for item in got if "reverb_rir" in item)
    # a name with prob 0 draws its chance and nothing else; rir_nums = 0 draws no index (_uniform's empty interval)
    a, b = np.random.default_rng(8), np.random.default_rng(8)
    assert simulate.draw_array_effects(3, P_EFFECTS, ["beep"], 0, a) == [{}, {}, {}]
    for _ in range(3):
        b.random()
    assert a.random() == b.random()
    a, b = np.random.default_rng(8), np.random.default_rng(8)
    one = simulate.draw_array_effects(1, {"reverb_rir": {"prob": [1.0]}}, ["reverb_rir"], 0, a)
    b.random()
    assert one == [{"reverb_rir": [True, 0]}] and a.random() == b.random()
    with pytest.raises(ValueError):
        simulate.draw_array_effects(1, P_EFFECTS, ["tempo"], 0, np.random.default_rng(0))
    # what it draws is what array_effects takes
    x = (np.random.default_rng(2).standard_normal(900) * 0.3).astype(np.float32)
    rirs = [np.array([1.0, 0.25], dtype=np.float32)] * 7
    for item in got[:10]:
        assert simulate.array_effects(x, item, rirs).shape == x.shape
