"""GPU parity of the vocoder's fused ResStack launches, one at a time, exactly as its plan builds them (vocoder.cpp: voc_resblock_params,
then plan_resblock / launch_resblock, through vfx_op_voc_resblock), against the float64 reference and the per-element bound of
tests/resstack_f64.py -- in the trunk forms, with the slopes, output sets and per-clip lengths of the 44.1 kHz plan and of its tuning
variants.  Two kinds of data: random reals at the product's slopes (0.01 inside the layer, 0.01 / 0.2 for the activated output), held
to the bound, and exact arithmetic (small integers, weights in {-1, 0, 1}, slopes 0.5 / 0.25), where the launch must return the
float64 values bit for bit.  Shapes come from the geometry the plan reports: around every tile seam, shorter than the dilation, one
position; clips of a batch end on a seam, one position past it, after one position -- x past a clip's end is NaN, the outputs past it
must still be NaN, and each clip must equal its batch-of-one launch bit for bit."""
import ctypes

import pytest
import torch

import resstack_f64 as R

pytestmark = pytest.mark.gpu

SLOPE, UP = 0.01, 0.2
NO_PERSISTENT_C64, NO_PAIRS, F32_TRUNK = 8, 16, 64
ALL_D = (1, 3, 9, 27, 81, 243, 729, 2187)
_ENGINES = {}


def _tuned(tuning):
    """A 16-bit handle with vfx_config.tuning = `tuning` (one per module run)."""
    if tuning not in _ENGINES:
        from conftest import TOL
        from voicefixer_main_amd.engine import Engine
        eng = Engine("cuda:0", config={"precision": 2, "tuning": tuning})
        eng.tol = TOL[2]
        _ENGINES[tuning] = eng
    return _ENGINES[tuning]


class Form:
    """How the plan runs the layers of one width on one handle: kernel family, trunk form, the outputs it stores."""

    def __init__(self, name, p, tuning, C, family, *, x16=False, asrc=False, pairs=(), singles=ALL_D, raw=True, act=False, lens_ok=True):
        self.name, self.p, self.tuning, self.C, self.family = name, p, tuning, C, family
        self.x16, self.asrc, self.pairs, self.singles, self.raw, self.act, self.lens_ok = x16, asrc, pairs, singles, raw, act, lens_ok

    def launches(self):
        """(dils, [(want_raw, want_act, act_slope)]): what the plan stores.  The last layer of a stack (d = 2187) in front of an upsampler
        also writes ya with the upsampler's slope -- on the fp16 trunk ya alone (run beside y too: the same bits); the wide layer writes
        ya for the next layer (the layer's own slope) and, last, for the upsampler."""
        inner = (self.raw, self.act, SLOPE)
        out = [((a, b), [inner]) for a, b in self.pairs]
        for d in self.singles:
            sets = [inner]
            if d == 2187 and self.p == 2 and self.tuning != NO_PAIRS:
                if self.asrc:
                    sets = [inner, (self.raw, True, UP)]
                elif self.x16 and self.C == 128:
                    sets = [(True, True, UP), (False, True, UP)]
                elif not (self.x16 and self.C == 64):   # (the C = 64 stack is the last one: the tail reads its raw trunk)
                    sets = [(True, True, UP)]
            out.append(((d,), sets))
        return out


FORMS = [
    Form("bf16-c64", 1, 0, 64, "k_resblock"),
    Form("bf16-c128", 1, 0, 128, "k_resblock"),
    Form("rw-c64", 2, 0, 64, "rw", x16=True, pairs=((1, 3), (9, 27)), singles=(81, 243, 729, 2187)),
    Form("r128-c128", 2, 0, 128, "r128", x16=True, pairs=((1, 3),), singles=(9, 27, 81, 243, 729, 2187)),
    Form("w64-c256", 2, 0, 256, "w64", x16=True, asrc=True, raw=False, act=True),
    Form("hionly-c64", 2, NO_PERSISTENT_C64, 64, "k_resblock"),
    Form("f32trunk-c64", 2, F32_TRUNK, 64, "rw", pairs=((1, 3), (9, 27)), singles=(81, 243, 729, 2187), lens_ok=False),
    Form("f32trunk-c128", 2, F32_TRUNK, 128, "r128", pairs=((1, 3),), singles=(9, 27, 81, 243, 729, 2187)),
    Form("f32trunk-c256", 2, F32_TRUNK, 256, "w64", asrc=True, act=True),
    Form("nopairs-c64", 2, NO_PAIRS, 64, "rw", x16=True, singles=(1, 3)),
    Form("nopairs-c128", 2, NO_PAIRS, 128, "r128", x16=True, singles=(1, 3)),
]
CASES = [(f, dils, sets) for f in FORMS for dils, sets in f.launches()]


def _handle(form, engine):
    """The `engine` fixture where its mode is the form's; None where that mode has no such launch."""
    return engine if {"fp32": 0, "split-bf16": 1, "fp16-vocoder": 2}[engine.tol['name']] == form.p else None


def _geo(form, T, dils):
    from voicefixer_main_amd import _lib
    out = (ctypes.c_int * 12)()
    assert _lib.load_test().vfx_plan_resblock_geometry_tuned(form.C, T, dils[0], dils[1] if len(dils) > 1 else 0, form.p, form.tuning, out) == 0
    return dict(zip(("fold", "TH", "W1", "TWo", "tiles_h", "tiles_w", "PW", "P", "tile_m", "rw", "patch_rows", "asrc"), out))


def _shapes(form, dils):
    """-> (Ts of the batch-of-one launches, T of the batches of three, their lengths): from the plan's geometry.
    1-D tiles: T in {1, 2, d, d + 1, TWo - 1, TWo, TWo + 1, 2 TWo + 1}; clips end at T, 1, TWo + 1 (one past the seam), TWo (on it),
    below the dilation.  Folded tiles (rows of d positions, TH rows per tile): k1 = the rows ONE tile row takes before one more position
    opens a second; T in {1, d - 1, d, d + 1, k1 d - 1, k1 d, k1 d + 1, col2 (the shortest T whose row 0 reaches the second tile
    column)}; the batch of three has k1 d + 1 positions -- tile rows of TH' rows -- and its clips end at T, 1, TH' d + 1, TH' d, d - 1,
    col2.  Every length of a batch is also run as a batch of one."""
    d = dils[0]
    g = _geo(form, 4096, dils)
    if not g["fold"]:
        two, dm = g["TWo"], max(dils)
        small = dm - 1 if dm > 1 else 2
        T3 = 2 * two + 1
        lens = ([T3, 1, two + 1], [two, small, two - 1])
        Ts = {1, 2, d, d + 1, dm, dm + 1, two - 1, two, two + 1, T3}
    else:
        # (resblock_rw picks the wider of two tile shapes by the tile count, so TH and TWo are those of each T's own geometry)
        k1 = min(k for k in range(1, 40) if _geo(form, k * d, dils)["tiles_h"] == 1 and _geo(form, k * d + 1, dils)["tiles_h"] >= 2)
        T3 = k1 * d + 1
        g3 = _geo(form, T3, dils)
        seam = g3["TH"] * d
        col2 = min(T for T in range(3, d) if T > _geo(form, T, dils)["TWo"] + 2)   # row 0 reaches the second tile column
        assert g3["tiles_h"] >= 2 and g3["tiles_w"] >= 2 and seam + 1 < T3 and _geo(form, col2, dils)["tiles_w"] >= 2
        lens = ([T3, 1, seam + 1], [seam, d - 1, col2])
        Ts = {1, d - 1, d, d + 1, k1 * d - 1, k1 * d, T3, col2}
    Ts |= set(lens[0]) | set(lens[1])
    return sorted(Ts), T3, lens


def _data(form, dils, kind, Tmax):
    C = form.C
    seed = 1000 * C + 10 * sum(dils) + len(dils)
    if kind == "exact":
        row = R.EXACT_ROW_SINGLE if len(dils) == 1 else R.EXACT_ROW_PAIR
        return R.exact_trunk(1, Tmax, C, seed)[0], tuple(R.exact_layer(C, seed + 1 + k, row) for k in range(len(dils))), 0.5, 0.25
    return R.random_trunk(1, Tmax, C, seed)[0], tuple(R.random_layer(C, seed + 1 + 4 * k) for k in range(len(dils))), SLOPE, None


def _family(form, info, what):
    want = {"k_resblock": (0, 0, 0), "rw": (1, 0, 0), "r128": (0, 1, 0), "w64": (0, 0, 1)}[form.family]
    assert (info["rw"], info["r128"], info["asrc"]) == want and info["x16"] == int(form.x16), (what, info)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(eng, form, dils, sets, kind):
    """Every shape of _shapes for one launch kind of one form, one kind of data."""
    p, C = form.p, form.C
    Ts, T3, lens_sets = _shapes(form, dils)
    master, layers, slope, act_exact = _data(form, dils, kind, max(Ts))
    tol = eng.tol['conv']
    l1, l2 = layers[0], (layers[1] if len(layers) == 2 else None)
    d2 = dils[1] if len(dils) == 2 else 0
    base, results = {}, []   # T -> reference at the first act_slope; per output set: T -> (y, ya)
    if kind == "exact":      # (one act_slope: sets that differ in it alone are one)
        sets = list(dict.fromkeys((r, a, UP) for r, a, _ in sets))
    for want_raw, want_act, act_slope in sets:
        act_slope = act_exact if kind == "exact" else act_slope
        kw = dict(layer2=l2, dil2=d2, slope=slope, act_slope=act_slope, want_raw=want_raw, want_act=want_act)
        one = {}
        results.append(one)
        for T in Ts:
            what = (form.name, dils, kind, T, want_raw, want_act, act_slope)
            if T not in base:
                base[T] = R.resstack_ref(master[:T], layers, dils, slope, act_slope, p, tol, x16=form.x16, asrc=form.asrc,
                                         bounds=kind != "exact")
                if kind == "exact":
                    assert R.exact_fits(base[T]), (what, "the exact data does not fit fp16")
            ref = R.with_act_slope(base[T], act_slope)
            eng.take_flags()
            y, ya, info = eng.op_voc_resblock(master[None, :T], l1, dils[0], **kw)
            assert eng.take_flags() == 0, (what, "a device flag was raised on O(1) data")
            _family(form, info, what)
            one[T] = (y, ya)
            for got, key, bar in ((y, "y", "bar_y16" if (form.x16 and not form.asrc) else "bar_y32"), (ya, "ya", "bar_ya")):
                if got is None:
                    continue
                got = got[0].cpu().double()
                if kind == "exact":
                    assert torch.equal(got, ref[key]), (what, key, (got - ref[key]).abs().max().item(),
                                                        (got != ref[key]).nonzero()[:4].tolist())
                else:
                    _check(got, ref[key], ref[bar], what + (key,))
        if not form.lens_ok:
            continue
        for lens in lens_sets:
            x = torch.full((3, T3, C), float("nan"))
            for b, Tb in enumerate(lens):
                x[b, :Tb] = master[:Tb]
            eng.take_flags()
            y, ya, info = eng.op_voc_resblock(x, l1, dils[0], lens=lens, **kw)
            # (x past each clip's end is NaN: nothing computed from it may raise VFX_FLAG_F16_SATURATED)
            assert eng.take_flags() == 0, (form.name, dils, kind, lens, "a device flag was raised from positions past a clip's end")
            _family(form, info, (form.name, dils, lens))
            for got, k in ((y, 0), (ya, 1)):
                if got is None:
                    continue
                for b, Tb in enumerate(lens):
                    what = (form.name, dils, kind, "lens", lens, b, "ya" if k else "y")
                    assert torch.isnan(got[b, Tb:]).all(), (what, "written past the clip's end")
                    assert torch.isfinite(got[b, :Tb]).all(), (what, "non-finite values inside the clip")
                    # the batch-of-one launch of this clip passed the clip's own bar above
                    assert torch.equal(_bits(got[b, :Tb]), _bits(one[Tb][k][0])), (what, "differs from the clip's batch-of-one launch")
    # ya does not depend on whether the raw output is stored beside it (the entry point checks that nothing else is written)
    with_ya = [r for (want_raw, want_act, a), r in zip(sets, results) if want_act and a == UP]
    if len(with_ya) == 2:
        for T in Ts:
            assert torch.equal(_bits(with_ya[0][T][1]), _bits(with_ya[1][T][1])), (form.name, dils, kind, T, "ya with / without y")


def _check(got, ref, bar, what):
    assert torch.isfinite(got).all(), (what, "non-finite values")
    err = (got - ref).abs()
    worst = (err / bar).max().item()
    assert worst <= 1.0, (what, "max |err| / bar = %.3g (err %.3g, bar %.3g)" % (worst, err.max().item(), bar.max().item()))


def _ids(cases):
    return ["%s-d%s" % (f.name, "_".join(str(d) for d in dils)) for f, dils, _ in cases]


FIXTURE_CASES = [c for c in CASES if c[0].tuning == 0]   # on the `engine` fixture, each in its own arithmetic mode
TUNED_CASES = [c for c in CASES if c[0].tuning != 0]     # the tuning variants of the 16-bit mode: explicit handles, run once
SKIP = "this form belongs to another arithmetic mode (fp32 has no fused ResStack kernel)"


@pytest.mark.parametrize("form,dils,sets", FIXTURE_CASES, ids=_ids(FIXTURE_CASES))
def test_random_reals_vs_fp64(engine, form, dils, sets):
    """Random reals at the product's slopes against the per-element bound of resstack_f64: holds the accumulation to fp32."""
    eng = _handle(form, engine)
    if eng is None:
        pytest.skip(SKIP)
    _run(eng, form, dils, sets, "real")


@pytest.mark.parametrize("form,dils,sets", TUNED_CASES, ids=_ids(TUNED_CASES))
def test_random_reals_vs_fp64_tuning_variants(form, dils, sets):
    """... under VFX_TUNE_NO_PERSISTENT_C64 (k_resblock's 16-bit form), VFX_TUNE_F32_TRUNK (fp32 and two-form trunks, ya beside y) and
    VFX_TUNE_NO_PAIRS (the layers of dilation 1 and 3 alone)."""
    _run(_tuned(form.tuning), form, dils, sets, "real")


@pytest.mark.parametrize("form,dils,sets", FIXTURE_CASES, ids=_ids(FIXTURE_CASES))
def test_exact_arithmetic_bitwise(engine, form, dils, sets):
    """Integers, weights in {-1, 0, 1}, biases in halves, slopes 0.5 / 0.25: every sum is exact in every mode (asserted on the CPU:
    exact_fits), so the launch returns the float64 values bit for bit -- no indexing, masking or slope defect survives."""
    eng = _handle(form, engine)
    if eng is None:
        pytest.skip(SKIP)
    _run(eng, form, dils, sets, "exact")


@pytest.mark.parametrize("form,dils,sets", TUNED_CASES, ids=_ids(TUNED_CASES))
def test_exact_arithmetic_bitwise_tuning_variants(form, dils, sets):
    _run(_tuned(form.tuning), form, dils, sets, "exact")


@pytest.mark.parametrize("form", [f for f in FORMS if f.lens_ok and f.tuning == 0], ids=lambda f: f.name)
def test_stage_lens_mul(engine, form):
    """Lengths in the stage's own unit (lens_mul = positions per vocoder frame: 49, 147, 441 at C = 256, 128, 64), lens = [3, 1, 2]."""
    eng = _handle(form, engine)
    if eng is None:
        pytest.skip(SKIP)
    _lens_mul(eng, form)


@pytest.mark.parametrize("form", [f for f in FORMS if f.lens_ok and f.tuning in (NO_PERSISTENT_C64, F32_TRUNK)], ids=lambda f: f.name)
def test_stage_lens_mul_tuning_variants(form):
    _lens_mul(_tuned(form.tuning), form)


def _lens_mul(eng, form):
    mul = {256: 49, 128: 147, 64: 441}[form.C]
    lens, T, C = [3, 1, 2], 3 * mul, form.C
    for kind in ("real", "exact"):
        master, layers, slope, act_exact = _data(form, (1,), kind, T)
        act_slope = act_exact if kind == "exact" else UP
        want_act = form.act or (form.p == 2 and form.raw and not form.x16)
        kw = dict(slope=slope, act_slope=act_slope, want_raw=form.raw, want_act=want_act)
        x = torch.full((3, T, C), float("nan"))
        for b, n in enumerate(lens):
            x[b, :n * mul] = master[:n * mul]
        y, ya, info = eng.op_voc_resblock(x, layers[0], 1, lens=lens, lens_mul=mul, **kw)
        _family(form, info, (form.name, "lens_mul"))
        for b, n in enumerate(lens):
            Tb = n * mul
            ref = R.resstack_ref(master[:Tb], layers, (1,), slope, act_slope, form.p, eng.tol['conv'], x16=form.x16, asrc=form.asrc,
                                 bounds=kind != "exact")
            y1, ya1, _ = eng.op_voc_resblock(master[None, :Tb], layers[0], 1, **kw)
            for got, solo, key, bar in ((y, y1, "y", "bar_y16" if (form.x16 and not form.asrc) else "bar_y32"), (ya, ya1, "ya", "bar_ya")):
                if got is None:
                    continue
                what = (form.name, kind, "lens_mul", mul, b, key)
                assert torch.isnan(got[b, Tb:]).all(), (what, "written past the clip's end")
                assert torch.equal(_bits(got[b, :Tb]), _bits(solo[0])), (what, "differs from the clip's batch-of-one launch")
                if kind == "exact":
                    assert R.exact_fits(ref) and torch.equal(got[b, :Tb].cpu().double(), ref[key]), what
                else:
                    _check(got[b, :Tb].cpu().double(), ref[key], ref[bar], what)


@pytest.mark.parametrize("dils", [(1,), (2187,), (9, 27)], ids=["d1", "d2187", "pair9_27"])
def test_persistent_blocks_across_clips(engine, dils):
    """resblock_rw (C = 64, 16-bit): 70001 positions, three clips of 70001, 255 and 35000 -- a block walks several tiles, skips the run
    of tiles past a clip's end (its prefetch with them) and crosses clip boundaries.  Each clip inside its own bar and, bit for bit,
    its batch-of-one launch; exact data returns the float64 values."""
    if engine.tol['name'] != 'fp16-vocoder':
        pytest.skip("the persistent kernel runs the C = 64 layers of the 16-bit mode")
    form = FORMS[2]
    C, T, lens = 64, 70001, [70001, 255, 35000]
    l2d = dict(dil2=dils[1]) if len(dils) == 2 else {}
    for kind in ("real", "exact"):
        master, layers, slope, act_exact = _data(form, dils, kind, T)
        kw = dict(layer2=layers[1] if len(dils) == 2 else None, slope=slope, want_raw=True, want_act=False, **l2d)
        x = torch.full((3, T, C), float("nan"))
        for b, Tb in enumerate(lens):
            x[b, :Tb] = master[:Tb]
        y, _, info = engine.op_voc_resblock(x, layers[0], dils[0], lens=lens, **kw)
        _family(form, info, ("persistent", dils))
        for b, Tb in enumerate(lens):
            what = ("persistent", dils, kind, b)
            ref = R.resstack_ref(master[:Tb], layers, dils, slope, act_exact or UP, 2, engine.tol['conv'], x16=True, bounds=kind != "exact")
            assert torch.isnan(y[b, Tb:]).all(), (what, "written past the clip's end")
            got = y[b, :Tb].cpu().double()
            if kind == "exact":
                assert R.exact_fits(ref) and torch.equal(got, ref["y"]), what
            else:
                _check(got, ref["y"], ref["bar_y16"], what)
            y1, _, _ = engine.op_voc_resblock(master[None, :Tb], layers[0], dils[0], **kw)
            assert torch.equal(_bits(y[b, :Tb]), _bits(y1[0])), (what, "differs from the clip's batch-of-one launch")


@pytest.mark.parametrize("form", [f for f in FORMS if f.p == 2 and f.tuning == 0 and not f.asrc], ids=lambda f: f.name)
def test_ya_with_and_without_the_raw_output(engine, form):
    """The last layer in front of an upsampler on the fp16 trunk stores ya alone (y == NULL): the same bits as beside y, with lengths
    too, and nothing else written (the entry point keeps both outputs between guard zones and fails the call otherwise)."""
    if engine.tol['name'] != 'fp16-vocoder':
        pytest.skip("the fp16 trunk exists in the 16-bit mode only")
    for dils in (((1, 3), (2187,)) if form.pairs else ((3,), (2187,))):
        Ts, T3, lens_sets = _shapes(form, dils)
        master, layers, slope, _ = _data(form, dils, "real", T3)
        kw = dict(layer2=layers[1] if len(dils) == 2 else None, dil2=dils[1] if len(dils) == 2 else 0, slope=slope, act_slope=UP)
        x = torch.full((3, T3, form.C), float("nan"))
        for b, Tb in enumerate(lens_sets[0]):
            x[b, :Tb] = master[:Tb]
        for xx, lens in ((master[None, :T3], None), (x, lens_sets[0])):
            _, ya_both, info = engine.op_voc_resblock(xx, layers[0], dils[0], lens=lens, want_raw=True, want_act=True, **kw)
            _, ya_only, _ = engine.op_voc_resblock(xx, layers[0], dils[0], lens=lens, want_raw=False, want_act=True, **kw)
            _family(form, info, (form.name, dils))
            assert torch.equal(_bits(ya_both), _bits(ya_only)), (form.name, dils, lens)


@pytest.mark.parametrize("tuning", [0, F32_TRUNK], ids=["f16-trunk", "f32-trunk"])
def test_older_entry_points_run_the_plans_launch(tuning):
    """vfx_op_resblock(fused) and vfx_op_resblock_pair take their parameter block from voc_resblock_params like vfx_op_voc_resblock: the
    same launch, so the same bits.  B = 2, T = 300: one or two tiles per clip at every width, the last one partial; d = 81 folds.  On the
    raw trunk (fp32, or fp16 widened) y is compared with y; the wide layer's fp16 trunk keeps no y, so the older entry point returns
    LeakyReLU^-1(ya), formed here as it forms it: v >= 0 ? v : v / slope in float32."""
    import numpy as np
    eng = _tuned(tuning)
    B, T = 2, 300
    for C in (64, 128, 256):
        x = R.random_trunk(B, T, C, 7 * C)
        la, lb = R.random_layer(C, 7 * C + 1), R.random_layer(C, 7 * C + 5)
        for d in (1, 27, 81):
            y_old = eng.op_resblock(x, *la, d, SLOPE, True)
            if C == 256 and tuning == 0:
                _, ya, info = eng.op_voc_resblock(x, la, d, slope=SLOPE, act_slope=SLOPE, want_raw=False, want_act=True)
                assert info["asrc"] == 1 and info["x16"] == 1, info
                v = ya.cpu().numpy()
                want = torch.from_numpy(np.where(v >= 0, v, v / np.float32(SLOPE)).astype(np.float32))
            else:
                want, _, info = eng.op_voc_resblock(x, la, d, slope=SLOPE, act_slope=SLOPE, want_raw=True, want_act=True)
                assert info["x16"] == int(tuning == 0), info
            assert torch.isfinite(y_old).all(), (C, d)
            assert torch.equal(_bits(y_old.cpu()), _bits(want.cpu())), (tuning, C, d, "single layer")
        for da, db in {64: ((1, 3), (9, 27)), 128: ((1, 3),), 256: ()}[C]:
            y_old = eng.op_resblock_pair(x, la, da, lb, db, SLOPE)
            want, _, info = eng.op_voc_resblock(x, la, da, layer2=lb, dil2=db, slope=SLOPE, act_slope=SLOPE, want_raw=True, want_act=True)
            assert info["x16"] == int(tuning == 0) and torch.isfinite(y_old).all(), (C, da, db, info)
            assert torch.equal(_bits(y_old.cpu()), _bits(want.cpu())), (tuning, C, da, db, "pair")


def test_refusals(engine):
    """Combinations the plan refuses are errors of the call, and nothing is launched."""
    if engine.tol['name'] == 'fp32':
        pytest.skip("fp32 has no fused ResStack kernel")
    C, T = 64, 300
    x = R.random_trunk(3, T, C, 1)
    la, lb = R.random_layer(C, 2), R.random_layer(C, 6)
    if engine.tol['name'] == 'split-bf16':
        with pytest.raises(RuntimeError):   # no activated output outside the 16-bit mode
            engine.op_voc_resblock(x, la, 1, want_act=True)
        with pytest.raises(RuntimeError):   # no layer pairs either
            engine.op_voc_resblock(x, la, 1, layer2=lb, dil2=3)
        return
    f32 = _tuned(F32_TRUNK)
    y, _, info = f32.op_voc_resblock(x, la, 1)
    assert info["rw"] == 1 and info["x16"] == 0 and torch.isfinite(y).all()
    with pytest.raises(RuntimeError):       # resblock_rw keeps no register for a clip's length on the fp32 trunk
        f32.op_voc_resblock(x, la, 1, lens=[300, 200, 1])
    with pytest.raises(RuntimeError):       # ... which keeps y beside ya
        f32.op_voc_resblock(x, la, 1, want_raw=False, want_act=True)
    with pytest.raises(RuntimeError):       # VFX_TUNE_NO_PAIRS: one launch per layer
        _tuned(NO_PAIRS).op_voc_resblock(x, la, 1, layer2=lb, dil2=3)
    with pytest.raises(RuntimeError):       # a pair the plan does not form
        engine.op_voc_resblock(x, la, 27, layer2=lb, dil2=81)
    x256 = R.random_trunk(1, T, 256, 3)
    with pytest.raises(RuntimeError):       # the wide layer on the fp16 trunk keeps no raw tensor
        engine.op_voc_resblock(x256, R.random_layer(256, 4), 1, want_raw=True, want_act=True)
    with pytest.raises(RuntimeError):       # a clip longer than the tensor
        engine.op_voc_resblock(x, la, 1, lens=[301, 1, 1])
