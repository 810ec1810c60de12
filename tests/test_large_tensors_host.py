"""CPU: the case table of the large-tensor launch tests (tests/large_cases.py) by arithmetic -- every case's tensor lies in
(2^31, 2^32 - 4096) bytes, a clip straddles byte 2^31 away from a tile's corner wherever the case says one does, and the planner
accepts each shape on the host and picks the family the case names; one batch more than the limit is refused with the library's error."""
import ctypes

import pytest

import large_cases as LC


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", LC.CASES, ids=_ids(LC.CASES))
def test_tensor_lies_in_the_upper_half_of_the_offset_range(case):
    assert LC.LO < case.nbytes < LC.HI, (case.name, case.nbytes)
    assert case.B % LC.P == 0
    b, pos, byte = case.straddle()
    assert LC.P <= b < case.B - 1, (case.name, b)        # byte 2^31 lies in a clip that is compared, and clips follow it
    if not case.straddles:
        # a power-of-two clip: byte 2^31 is the first byte of clip b, nothing straddles it (the *-mel cases do)
        assert case.clip_bytes & (case.clip_bytes - 1) == 0 and (pos, byte) == (0, 0), (case.name, pos, byte)
    else:
        assert pos > 0 and all(pos % t for t in case.tiles), (case.name, pos, case.tiles)
    assert len({c.name for c in LC.CASES}) == len(LC.CASES)


def _block2d_tile(C, H, W, kind=0):
    from voicefixer_main_amd import _lib
    out = (ctypes.c_int * 8)()
    assert _lib.load_test().vfx_plan_block2d_geometry(C, H, W, kind, 0, out) == 0
    return out[0], out[2]      # TH, TWo: the outputs of one tile


def _conv_tile(H, W):
    from voicefixer_main_amd import _lib
    taps = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    dh, dw = (ctypes.c_int * 9)(*[t[0] for t in taps]), (ctypes.c_int * 9)(*[t[1] for t in taps])
    out = (ctypes.c_int * 6)()
    assert _lib.load_test().vfx_plan_conv_geometry(H, W, 9, dh, dw, out) == 0
    return out[0], out[1]      # TH, TW


@pytest.mark.parametrize("case", LC.UNET_CASES, ids=_ids(LC.UNET_CASES))
def test_planner_accepts_the_unet_cases(case):
    """vfx_plan_unet_piece at the case's B: the family the case names; a straddling clip meets byte 2^31 inside a tile of that
    family's geometry, not on its first pixel."""
    from voicefixer_main_amd.engine import Engine
    a = case.args
    H, W = a["hw"]
    arg = {"pool": case.large[-1], "final": 1}.get(a["piece"], int(a["piece"].endswith(".up")))
    launches = Engine.plan_unet_piece(a["piece"], case.B, H, W, arg=arg, precision=a["precision"])
    assert [l["family"] for l in launches] == a["families"], launches
    if case.straddles:
        _, pos, _ = case.straddle()
        row, col = divmod(pos, case.large[1])
        TH, TW = _block2d_tile(case.large[-1], H, W) if a["families"] == ["k_block2d32"] else _conv_tile(H, W)
        assert (row % TH, col % TW) != (0, 0) and col % TW != 0, (case.name, row, col, TH, TW)


@pytest.mark.parametrize("case", LC.VOC_CASES, ids=_ids(LC.VOC_CASES))
def test_planner_accepts_the_vocoder_cases(case):
    from voicefixer_main_amd import _lib
    lib = _lib.load_test()
    a = case.args
    if case.kind == "voc_resblock":
        out = (ctypes.c_int * 12)()
        assert lib.vfx_plan_resblock_geometry_tuned(a["C"], LC.VT, a["dil"], 0, a["precision"], 0, out) == 0
        g = dict(zip(("fold", "TH", "W1", "TWo", "tiles_h", "tiles_w", "PW", "P", "tile_m", "rw", "patch_rows", "asrc"), out))
        assert (g["fold"], g["rw"], g["asrc"]) == (a["fold"], 0, 0), g
        _, pos, _ = case.straddle()
        if g["fold"]:     # rows of `dil` positions, tiles of TH rows x TWo columns
            row, col = divmod(pos, a["dil"])
            assert col % g["TWo"] != 0, (pos, g)
        else:
            assert pos % g["TWo"] != 0, (pos, g)
    elif case.kind == "voc_conv1d":
        assert lib.vfx_plan_voc_conv_kernel(a["C"], a["C"], LC.VT, a["dil"], 0, a["precision"], 0) == 0   # plain k_conv
        assert (2 * a["dil"] + 128 > 192 and a["dil"] >= 16) == (a["dil"] == LC.FOLDED)                # plan.cpp set_conv1d_geometry
    elif case.kind == "voc_upsample":
        assert lib.vfx_plan_voc_upsampler_kernel(a["Cin"], a["Cin"] // 2, a["stride"], a["T"], a["precision"], 0) == 0   # the phased k_conv
        assert case.large == (a["stride"] * a["T"], a["Cin"] // 2)


@pytest.mark.parametrize("what,piece,B,hw,precision,err", LC.REFUSED_UNET, ids=[r[0] for r in LC.REFUSED_UNET])
def test_planner_refuses_one_batch_more(what, piece, B, hw, precision, err):
    """B - 1 clips stay below 2^32 - 4096 bytes and are planned; B clips reach it and are refused by the host checks."""
    from voicefixer_main_amd.engine import Engine
    C = {"enc1.2": 32, "enc2.2": 64, "enc3.2": 128}[piece]
    assert (B - 1) * hw[0] * hw[1] * C * 4 < LC.HI <= B * hw[0] * hw[1] * C * 4
    assert Engine.plan_unet_piece(piece, B - 1, hw[0], hw[1], precision=precision)
    with pytest.raises(RuntimeError, match=err):
        Engine.plan_unet_piece(piece, B, hw[0], hw[1], precision=precision)
