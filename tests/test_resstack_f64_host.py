"""CPU checks of tests/resstack_f64.py, the reference and bound that tests/test_gpu_resstack_launches.py holds the fused ResStack
launches to: the reference is the oracle's layer when nothing is rounded, a torch emulation of the kernel (operands rounded as the
mode does, fp32 accumulation) stays inside the bar in every mode and trunk form, and each defect planted into that emulation exceeds
the bar at the elements it touches -- so the GPU tests can fail.  Tile positions come from the plan (vfx_plan_resblock_geometry_tuned)."""
import ctypes

import pytest
import torch

import resstack_f64 as R
from conftest import TOL

SLOPE, UP = 0.01, 0.2
GEO = ("fold", "TH", "W1", "TWo", "tiles_h", "tiles_w", "PW", "P", "tile_m", "rw", "patch_rows", "asrc")


def _geometry(C, T, dil, dil2, p, tuning=0):
    from voicefixer_main_amd import _lib
    out = (ctypes.c_int * 12)()
    assert _lib.load_test().vfx_plan_resblock_geometry_tuned(C, T, dil, dil2, p, tuning, out) == 0
    return dict(zip(GEO, out))


# (id, p, C, tuning, x16, asrc, packed): the forms of the 44.1 kHz plan and of its tuning variants
FORMS = [
    ("c64-bf16", 1, 64, 0, False, False, False),
    ("c128-bf16", 1, 128, 0, False, False, False),
    ("c64-rw", 2, 64, 0, True, False, True),
    ("c64-hionly", 2, 64, 8, False, False, False),
    ("c128-r128", 2, 128, 0, True, False, True),
    ("c256-w64", 2, 256, 0, True, True, True),
    ("c64-rw-f32", 2, 64, 64, False, False, True),
    ("c128-r128-f32", 2, 128, 64, False, False, True),
    ("c256-w64-f32", 2, 256, 64, False, True, True),
]
IDS = [f[0] for f in FORMS]


def _pairs(form):
    _, p, C, tuning, _, asrc, _ = form
    if p != 2 or asrc or (tuning & 8):
        return []
    return [(1, 3), (9, 27)] if C == 64 else [(1, 3)]


def test_reference_is_the_oracle_layer_when_nothing_rounds():
    """p = 0 (operands are the fp32 values themselves): the reference of a layer and of a pair is oracle.vocoder's ResStack in float64.
    A single layer of dilation d is the oracle's two-layer stack whose first layer has zero weights."""
    C, T = 64, 61
    x = R.random_trunk(1, T, C, 1)[0]
    la, lb = R.random_layer(C, 10), R.random_layer(C, 20)
    zero = tuple(torch.zeros_like(t) for t in la)
    for d2 in (3, 27, 81):
        ref = R.resstack_ref(x, (la, lb), (1, d2), SLOPE, UP, 0, 1.0)
        assert (ref["y"] - R.oracle_layers(x, (la, lb), (1, d2), SLOPE)).abs().max() < 1e-12
        one = R.resstack_ref(x, (lb,), (d2,), SLOPE, UP, 0, 1.0)
        assert (one["y"] - R.oracle_layers(x, (zero, lb), (1, d2), SLOPE)).abs().max() < 1e-12
        assert torch.equal(one["ya"], torch.where(one["y"] > 0, one["y"], one["y"] * UP))
    one = R.resstack_ref(x, (la,), (1,), SLOPE, UP, 0, 1.0)
    assert (one["y"] - R.oracle_layers(x, (la,), (1,), SLOPE)).abs().max() < 1e-12


def _cases(form):
    """(dils, T, Tb): a 1-D layer and a folded one (a clip that ends one position into the second tile, the row past it holding the
    neighbour's data), and the pairs of the form."""
    _, p, C, tuning, _, _, _ = form
    out = []
    for d in (1, 243):
        g = _geometry(C, 4096, d, 0, p, tuning)
        seam = g["TH"] * d if g["fold"] else g["TWo"]
        out.append(((d,), seam + 40, seam + 1))
    for da, db in _pairs(form):
        g = _geometry(C, 4096, da, db, p, tuning)
        out.append(((da, db), g["TWo"] + 70, g["TWo"] + 1))
    return out


def _check(y, ya, ref, p, x16, asrc, what):
    bar_y = ref["bar_y16"] if (x16 and not asrc) else ref["bar_y32"]
    if not (x16 and asrc):   # (the wide layer on the fp16 trunk stores ya alone)
        assert ((y.double() - ref["y"]).abs() <= bar_y).all(), (what, "y", ((y.double() - ref["y"]).abs() / bar_y).max().item())
    if p == 2:               # (the activated output exists in the 16-bit mode only)
        assert ((ya.double() - ref["ya"]).abs() <= ref["bar_ya"]).all(), (what, "ya", ((ya.double() - ref["ya"]).abs() / ref["bar_ya"]).max().item())


@pytest.mark.parametrize("form", FORMS, ids=IDS)
def test_emulation_stays_inside_the_bar(form):
    name, p, C, tuning, x16, asrc, packed = form
    tol = TOL[p]["conv"]
    for i, (dils, T, Tb) in enumerate(_cases(form)):
        x = R.random_trunk(1, T, C, 100 + i)[0]
        layers = tuple(R.random_layer(C, 200 + 10 * i + 4 * k) for k in range(len(dils)))
        for act_slope in (SLOPE, UP):
            ref = R.resstack_ref(x[:Tb], layers, dils, SLOPE, act_slope, p, tol, x16=x16, asrc=asrc)
            y, ya = R.emulate(x, Tb, layers, dils, SLOPE, act_slope, p, x16=x16, asrc=asrc, packed=packed)
            _check(y, ya, ref, p, x16, asrc, (name, dils, act_slope))
            if p == 2 and packed:   # ... and in the other activation form of the 16-bit mode (fp32 LeakyReLU, then fp16)
                y, ya = R.emulate(x, Tb, layers, dils, SLOPE, act_slope, p, x16=x16, asrc=asrc, packed=False)
                _check(y, ya, ref, p, x16, asrc, (name, dils, act_slope, "fp32 activation"))


def _aligned_case(C, T):
    """Data on which a coarser rounding of h adds up instead of averaging out: w1 = 0, so h = b1 in every position; b1 = 1 + 2^-8 - 2^-10 is
    an fp16 number (and a hi + lo pair) that bf16 rounds down by 2^-8 - 2^-10; w2 >= 0.  The bar's conv(dg, |w2q|) term is the worst
    case of exactly such alignment for ONE rounding of the operand form; bf16's is eight times the fp16 one and 2^8 times the pair's."""
    w1, _, w2, b2 = R.random_layer(C, 900)
    b1 = torch.full((C,), 1.0 + 2.0 ** -8 - 2.0 ** -10)
    return R.random_trunk(1, T, C, 901)[0], (torch.zeros_like(w1), b1, w2.abs(), b2)


# (layer pairs and the activated output exist in some forms only)
PLANTED = [(f, d) for d in R.DEFECTS for f in FORMS if not (d == "swap_pair" and not _pairs(f)) and not (d == "ya_slope" and f[1] != 2)]


@pytest.mark.parametrize("form,defect", PLANTED, ids=["%s-%s" % (d, f[0]) for f, d in PLANTED])
def test_planted_defect_exceeds_the_bar(form, defect):
    """Each defect of resstack_f64.DEFECTS, planted into the emulation of each form, leaves the bar at every position it touches -- in
    most of that position's channels: one channel's sum of random terms can land near zero, and the 16-bit bar of a 256-channel layer
    is its worst-case sum of 768 operand roundings -- and nowhere else does the emulation leave it."""
    name, p, C, tuning, x16, asrc, packed = form
    tol = TOL[p]["conv"]
    d = 3
    dils = (1, 3) if defect == "swap_pair" else (d,)
    g = _geometry(C, 4096, dils[0], dils[1] if len(dils) > 1 else 0, p, tuning)
    seam = g["TWo"]                      # first output column of the second tile
    T, Tb = seam + 60, seam + 30
    x = R.random_trunk(1, T, C, 300)[0]
    layers = tuple(R.random_layer(C, 400 + 4 * k) for k in range(len(dils)))
    if defect == "h_bf16":
        x, lay = _aligned_case(C, T)
        layers = (lay,)
    ref = R.resstack_ref(x[:Tb], layers, dils, SLOPE, UP, p, tol, x16=x16, asrc=asrc)
    y, ya = R.emulate(x, Tb, layers, dils, SLOPE, UP, p, x16=x16, asrc=asrc, packed=packed, defect=defect, where=seam)
    bar_y = ref["bar_y16"] if (x16 and not asrc) else ref["bar_y32"]
    bad_y = (y.double() - ref["y"]).abs() > bar_y
    bad_ya = (ya.double() - ref["ya"]).abs() > ref["bar_ya"]
    touched = torch.zeros(Tb, C, dtype=torch.bool)
    if defect == "h_past_end":
        touched[Tb - 1] = True             # conv2's last tap of the clip's last position reads h[Tb]
    elif defect == "x_past_end":
        touched[Tb - d - 1:] = True        # h of the last d positions saw x past the end; conv2 spreads it by one
    elif defect == "ya_slope":
        touched = ref["y"] < -10 * ref["bar_ya"]
        assert touched.any() and not bad_y.any()
        assert bad_ya[touched].all() and not bad_ya[ref["y"] >= 0].any()
        return
    elif defect == "drop_tap":
        touched[seam] = True
    else:                                  # res_shift, h_bf16, swap_pair: every element
        touched[:] = True
    def exceeds(bad, what):
        rows = touched.any(dim=1)
        assert (bad & touched).any(dim=1)[rows].all(), (name, defect, what, "a touched position stays inside the bar")
        assert bad[touched].float().mean() > 0.5, (name, defect, what, bad[touched].float().mean().item())
        assert not bad[~touched].any(), (name, defect, what, "the bar is left where the defect does not reach")

    if not (asrc and x16):   # (the wide layer on the fp16 trunk stores ya alone)
        exceeds(bad_y, "y")
    if p == 2:
        exceeds(bad_ya, "ya")


def test_exact_data_fits_fp16():
    """The exact-arithmetic data of the GPU test: every intermediate of a layer and of a pair is an fp16 number at the densities used."""
    for C in (64, 128, 256):
        x = R.exact_trunk(1, 300, C, 5)[0]
        ref = R.resstack_ref(x, (R.exact_layer(C, 6, R.EXACT_ROW_SINGLE),), (3,), 0.5, 0.25, 2, 1.0, x16=True, asrc=C == 256)
        assert R.exact_fits(ref)
        assert torch.equal(ref["y"], R.oracle_layers(x, (tuple(torch.zeros_like(t) for t in R.exact_layer(C, 6)),
                                                         R.exact_layer(C, 6, R.EXACT_ROW_SINGLE)), (1, 3), 0.5))
    for C in (64, 128):
        x = R.exact_trunk(1, 300, C, 7)[0]
        layers = (R.exact_layer(C, 8, R.EXACT_ROW_PAIR), R.exact_layer(C, 9, R.EXACT_ROW_PAIR))
        ref = R.resstack_ref(x, layers, (1, 3), 0.5, 0.25, 2, 1.0, x16=True)
        assert R.exact_fits(ref)
        assert torch.equal(ref["y"], R.oracle_layers(x, layers, (1, 3), 0.5))
        y, ya = R.emulate(x, 300, layers, (1, 3), 0.5, 0.25, 2, x16=True, packed=True)
        assert torch.equal(y.double(), ref["y"]) and torch.equal(ya.double(), ref["ya"])


def test_entry_point_is_declared_and_bound():
    """vfx_op_voc_resblock: declared in include/vfx_test.h, bound with as many arguments in _lib.TEST_SIGNATURES, wrapped by Engine, and
    built through the plan's builder (the plan itself fills no ResBlockParams of a 1-D layer by hand)."""
    import os
    import re
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import Engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"\bint vfx_op_voc_resblock\(([^;]*)\);", open(os.path.join(root, "include", "vfx_test.h")).read())
    assert m and len(m.group(1).split(",")) == 25 == len(_lib.TEST_SIGNATURES["vfx_op_voc_resblock"][1])
    assert hasattr(_lib.load_test(), "vfx_op_voc_resblock") and len(Engine.RESBLOCK_INFO) == 12 and hasattr(Engine, "op_voc_resblock")
    voc = open(os.path.join(root, "voicefixer_main_amd", "csrc", "vocoder.cpp")).read()
    plan = voc[voc.index("void build_vocoder("):]
    assert plan.count("voc_resblock_params(") == 2 and "ResBlockParams rp" not in plan
    dbg = open(os.path.join(root, "voicefixer_main_amd", "csrc", "ops_debug.cpp")).read()
    entry = dbg[dbg.index('extern "C" int vfx_op_voc_resblock('):]
    assert "voc_resblock_params(" in entry[:entry.index("// ---- the ResUNet plans")]
