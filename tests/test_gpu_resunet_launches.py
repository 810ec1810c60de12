"""GPU parity of the ResUNet plan's launches, one piece at a time, exactly as the plan builds them (resunet.cpp: build_unet_piece runs
the member functions of TrunkBuilder that the product plan runs, on the handle's own packed weights), against float64 torch on the
operands the launch multiplies (tests/resunet_pieces_f64.py).

The bar is the summation bound of tests/launch_parity_f64.py, per element:

    |y - ref| <= (n f + 2) u32 (S + |bias| + |residual|)  [+ 2^-17 S in split-bf16: the omitted lo*lo products]  + E

n = taps x channels over all K segments of the launch, f = 3 MFMA products per product in split-bf16 and 1 in fp32, S the float64
convolution of the |operands|, E what the launch's own fp32 prologue (BatchNorm folded in fp32, one multiply-add, LeakyReLU) may
differ from the reference's, pushed through the |weights| (resunet_pieces_f64.prologue derives it).  Never looser than
TOL[p]['conv'] * max(1, max |ref|).  Precision 2 runs the ResUNets as precision 1: its handle is held to the split-bf16 bar.

Two-launch blocks (C >= 128, every block with a shortcut above C = 32, everything in fp32) are checked launch by launch: conv1's
stored output h -- LeakyReLU(bn2(.)) in the operand form conv2 reads -- against its reference (bound of conv1 x |bn2 scale|, the
affine's rounding, then launch_parity_f64._act_bar for the activation and the storage rounding), and conv2 on the h the GPU stored,
which then carries no error of its own.

Single-launch blocks (resblock.hip G2 / IN1 / SC2, block2d32.hip) keep h in LDS.  Read off the kernels: h is held ACTIVATED,
LeakyReLU(bn2 scale * acc + bn2 shift) evaluated in fp32 and split into the hi + lo bf16 pair (resblock.hip phase 2 and the IN1
loop; block2d32.hip "split-bf16 operands") -- the same form a two-launch conv1 stores.  conv2's reference then runs on the float64
activated h and its bar carries h's error: F.conv2d(bar_h_act, |w2 operands|) is added, bar_h_act from _act_bar for that form.  No
bar comes from a kernel's output.

The entry block's conv1 and shortcut are nine and one plain fp32 multiply-adds per output in every mode (f = 1, fp32 operands).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resunet_pieces_f64 as R
from conftest import TOL
from launch_parity_f64 import U32, _act_bar, _bar, _check, _rand
from resunet_pieces_f64 import nchw
from voicefixer_main_amd.engine import MODEL_UNET_MEL, MODEL_UNET_SPEC

pytestmark = pytest.mark.gpu

B = 2
FUSED_SHAPES = [(1, 1), (14, 14), (15, 29), (17, 3), (64, 127)]   # around the 16 x 16 h tile (14 x 14 outputs); (64, 127): level 1 at Tpad = 64


def _mode(engine):
    """-> (arithmetic mode of the ResUNets on this handle, its conv bar)."""
    p = min({"fp32": 0, "split-bf16": 1, "fp16-vocoder": 2}[engine.tol['name']], 1)
    return p, TOL[p]['conv']


def _src(shape, seed, scale=1.0, shift=0.0):
    """Random activations with negative values in a regular pattern: both branches of every LeakyReLU / ReLU prologue are taken."""
    x = _rand(shape, seed, scale) + shift
    x[:, ::3, ::2] = -x[:, ::3, ::2].abs()
    return x


def _bound(d, p, tol, more=0.0):
    b, cap = _bar(d["ref"], d["S"], d["n"], p, tol, extra=d["extra"])
    return torch.minimum(b + d["E"] + more, torch.full_like(b, cap))


def _h_bound(sd, prefix, c1, bar_h, p, tol):
    """-> (float64 activated h, its bound in the stored / LDS form)."""
    ha, scale_abs, affine = R.h_activated(sd, prefix, c1["ref"])
    return ha, _act_bar(ha, bar_h * scale_abs + affine, 1.0, p, tol * max(1.0, float(ha.abs().max())))


def _families(launches):
    return [l["family"] for l in launches]


def _block_case(eng, sd, piece, H, W, seed, short_clips=(0,), model=MODEL_UNET_MEL, B=B, run=None, plan_B=None):
    """One ConvBlockRes piece of `model` over (B, H, W): every launch against its reference; -> the launches of each run.
    run: stands in for eng.op_unet_piece (tests/test_gpu_large_tensors.py: the same clips repeated to a batch of plan_B, of which it
    hands back the first B)."""
    p, tol = _mode(eng)
    prefix = R.block_prefix(piece)
    cin = sd[prefix + ".conv1.weight"].shape[1]
    nsrc = 2 if piece.startswith("dec") and piece.endswith(".1") else 1
    srcs = [_src((B, H, W, cin // nsrc), seed + i) for i in range(nsrc)]
    c1 = R.conv1(sd, prefix, srcs, p)
    ha, bar_ha = _h_bound(sd, prefix, c1, _bound(c1, p, tol), p, tol)
    runs = []
    for sc in short_clips:
        (y,), h, launches = (run or eng.op_unet_piece)(piece, srcs, short_clip=sc, model=model)
        what = (piece, H, W, sc, _families(launches))
        if h is None:   # one launch: h stayed in LDS
            c2 = R.conv2(sd, prefix, ha, srcs, p)
            _check(nchw(y.cpu()), c2["ref"], _bound(c2, p, tol, more=F.conv2d(bar_ha, c2["w_abs"], padding=1)), what + ("y",))
        else:
            assert h[0] == "act" and _families(launches) == ["k_conv", "k_conv"], what
            hg = nchw(h[1].cpu())
            _check(hg, ha, bar_ha, what + ("h",))
            c2 = R.conv2(sd, prefix, hg.double(), srcs, p)   # conv2 on its own input: the h the GPU stored, already in operand form
            _check(nchw(y.cpu()), c2["ref"], _bound(c2, p, tol), what + ("y",))
        assert launches == eng.plan_unet_piece(piece, plan_B or B, H, W, short_clip=sc, precision=eng.cfg.precision, tuning=eng.cfg.tuning), what
        runs.append(launches)
    return runs


# ---------------------------------------------------------------------------------------------------------------------------------
# level 1: the single-launch blocks (two launches each in fp32)
# ---------------------------------------------------------------------------------------------------------------------------------
def _entry_case(eng, sd, H, W, model=MODEL_UNET_MEL, B=B, run=None):
    """encoder_block1.conv_block1 of `model` on a (B, H, W) plane; -> the launches' families."""
    p, tol = _mode(eng)
    prefix = "encoder_block1.conv_block1"
    x = _src((B, H, W), 11 * H + W, 1.2, -2.5)   # log-mel-like
    c1, sc = R.entry_conv1(sd, x, p)
    bar_h = _bound(c1, 0, tol)
    (y,), h, launches = (run or eng.op_unet_piece)("entry", [x], model=model)
    what = ("entry", H, W, _families(launches))
    if h is None:
        assert _families(launches) == ["k_resblock_in1"], what
        ha, bar_ha = _h_bound(sd, prefix, c1, bar_h, p, tol)
        c2 = R.conv2(sd, prefix, ha, [], p, residual=sc)
        _check(nchw(y.cpu()), c2["ref"], _bound(c2, p, tol, more=F.conv2d(bar_ha, c2["w_abs"], padding=1)), what + ("y",))
    else:
        assert h[0] == "raw" and _families(launches) == ["small", "k_conv"], what
        hg = nchw(h[1].cpu())
        _check(hg, c1["ref"], bar_h, what + ("h",))
        a, err = R.prologue(hg, R.fold_bn(sd, prefix + ".bn2"), R.SLOPE, p)   # conv2's own prologue on the raw h the GPU stored
        c2 = R.conv2(sd, prefix, a, [], p, residual=sc)
        _check(nchw(y.cpu()), c2["ref"], _bound(c2, p, tol, more=F.conv2d(err, c2["w_abs"], padding=1)), what + ("y",))
    return _families(launches)


@pytest.mark.parametrize("H,W", FUSED_SHAPES)
def test_entry_block(engine, unet_sd, H, W):
    """The fused IN1 launch, or k_conv_c1 + k_conv in fp32."""
    p, _ = _mode(engine)
    assert _entry_case(engine, unet_sd, H, W) == (["k_resblock_in1"] if p == 1 else ["small", "k_conv"])


def test_level1_two_launch_forms_in_split_bf16(unet_sd):
    """VFX_TUNE_NO_FUSED_UNET on a split-bf16 handle: the entry block as k_conv_c1 + k_conv, the C = 32 / 64 blocks (identity, and two
    sources with shortcut segments) as two k_conv launches each, an upsampler as four parity launches."""
    from voicefixer_main_amd import _lib
    eng = _engine(1, _lib.TUNE_NO_FUSED_UNET, unet_sd)
    for i, (H, W) in enumerate([(15, 29), (17, 3)]):
        assert _entry_case(eng, unet_sd, H, W) == ["small", "k_conv"]
        for piece in ("enc1.2", "dec6.1", "enc2.2"):
            (launches,) = _block_case(eng, unet_sd, piece, H, W, 160 + i)
            assert _families(launches) == ["k_conv", "k_conv"], (piece, H, W, launches)
    for prune_w in (False, True):
        assert _up_case(eng, unet_sd, 6, 5, 17, prune_w, 170) == ["k_conv"] * 4


@pytest.mark.parametrize("piece", ["enc1.2", "enc1.4", "dec6.1", "dec6.3", "after", "enc2.2", "dec5.2"])
def test_fused_block(engine, unet_sd, piece):
    """The C = 32 blocks (identity: k_block2d32; two sources with 1x1 shortcuts: k_resblock SC2) and the C = 64 identity block
    (k_resblock G2) over FUSED_SHAPES; in fp32 each is two k_conv launches."""
    p, _ = _mode(engine)
    seen = set()
    for i, (H, W) in enumerate(FUSED_SHAPES):
        (launches,) = _block_case(engine, unet_sd, piece, H, W, 100 + i)
        seen.add(tuple(_families(launches)))
    # (the persistent C = 32 kernel takes the shapes its tiles fit, k_resblock's 16 x 16 tiles the others: FUSED_SHAPES has both)
    want = {"dec6.1": {("k_resblock_two_src",)}, "enc2.2": {("k_resblock",)}, "dec5.2": {("k_resblock",)}}.get(piece, {("k_block2d32",), ("k_resblock",)})
    assert seen == ({("k_conv", "k_conv")} if p == 0 else want), (piece, seen)


def test_level1_blocks_on_16x16_tiles(unet_sd):
    """VFX_TUNE_OLD_BLOCK2D: the C = 32 identity block on k_resblock's 16 x 16 h tiles instead of the persistent kernel."""
    from voicefixer_main_amd import _lib
    eng = _engine(1, _lib.TUNE_OLD_BLOCK2D, unet_sd)
    for i, (H, W) in enumerate(FUSED_SHAPES):
        (launches,) = _block_case(eng, unet_sd, "enc1.3", H, W, 150 + i)
        assert _families(launches) == ["k_resblock"], (H, W, launches)


# ---------------------------------------------------------------------------------------------------------------------------------
# the deep levels: two launches, split-K
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", sorted(R.DEEP_CASES))
def test_two_launch_block(engine, unet_sd, piece):
    """Every deep block at its own level shapes with short_clip 1, 0 and -2 (the three split-K rules): conv1 with one or two segments
    into the activated h, conv2 with the residual or with the shortcut segments plus bias, whatever ksplit the planner picks."""
    for i, (H, W) in enumerate(R.DEEP_CASES[piece]):
        for launches in _block_case(engine, unet_sd, piece, H, W, 200 + i, short_clips=R.SHORT_CLIPS):
            assert _families(launches) == ["k_conv", "k_conv"] and launches[0]["out_act"] and not launches[1]["out_act"], (piece, H, W, launches)


def test_deep_cases_cover_every_split_k(engine):
    """The cases above reach ksplit 1, 2, 4 and 8, each with an activated output and with shortcut segments plus bias, on this
    handle's precision and tuning (test_two_launch_block asserts that every run launched what this query says)."""
    act, shortcut = R.splitk_coverage(lambda piece, H, W, sc: engine.plan_unet_piece(piece, B, H, W, short_clip=sc, precision=engine.cfg.precision,
                                                                                     tuning=engine.cfg.tuning))
    assert act >= {1, 2, 4, 8} and shortcut >= {1, 2, 4, 8}, (act, shortcut)


# ---------------------------------------------------------------------------------------------------------------------------------
# upsamplers
# ---------------------------------------------------------------------------------------------------------------------------------
UP_FALLBACK = [(1, 1), (2, 1), (1, 3)]            # four parity launches (the mel net's decoder 1 at one padded chunk: (1, 1))
UP_PHASED = [(2, 2), (2, 3), (5, 17), (16, 31)]   # one launch of four phases


def _up_case(eng, sd, d, H, W, prune_w, seed, model=MODEL_UNET_MEL, run=None):
    p, tol = _mode(eng)
    cin = sd["decoder_block%d.conv1.weight" % d].shape[0]
    x = _src((B, H, W, cin), seed)
    r = R.upsample(sd, "decoder_block%d" % d, x, prune_w, p)
    (y,), _, launches = (run or eng.op_unet_piece)("dec%d.up" % d, [x], arg=int(prune_w), model=model)
    assert y.shape == (B, 2 * H, 2 * W if prune_w else 2 * W + 1, r["ref"].shape[1])
    # (the output started as NaN: _check requires every element finite -- no pixel unwritten; a write past the last column would land in
    # the next row's first pixels and fail there)
    _check(nchw(y.cpu()), r["ref"], _bound(r, p, tol), ("dec%d.up" % d, H, W, prune_w, _families(launches)))
    return _families(launches)


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_upsampler(engine, unet_sd, d):
    """Every decoder's ConvTranspose2d with the handle's own wT tables, both output widths: the four-parity fallback and the one-launch
    four-phase form."""
    for prune_w in (False, True):
        for i, (H, W) in enumerate(UP_FALLBACK):
            assert _up_case(engine, unet_sd, d, H, W, prune_w, 300 + i) == ["k_conv"] * 4
        for i, (H, W) in enumerate(UP_PHASED):
            assert _up_case(engine, unet_sd, d, H, W, prune_w, 310 + i) == ["k_conv_phased"]


def test_two_launch_upsamplers(engine, unet_sd):
    """VFX_TUNE_TWO_LAUNCH_UPSAMPLERS: one phased launch per output row class, once per output width."""
    from voicefixer_main_amd import _lib
    eng = _engine(engine.cfg.precision, _lib.TUNE_TWO_LAUNCH_UPSAMPLERS, unet_sd)
    for prune_w in (False, True):
        assert _up_case(eng, unet_sd, 3, 5, 17, prune_w, 320) == ["k_conv_phased"] * 2


# ---------------------------------------------------------------------------------------------------------------------------------
# precision 2 runs the ResUNets as precision 1
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine(precision, tuning, sd, model=MODEL_UNET_MEL):
    from voicefixer_main_amd.engine import Engine
    eng = Engine("cuda:0", config={"precision": precision, "tuning": tuning})
    eng.load_state_dict(model, sd)
    eng.tol = TOL[precision]
    return eng


def test_precision_2_gives_precision_1_bits(unet_sd):
    """One piece of each kernel family: a precision-2 handle gives the precision-1 handle's bits (outputs and stored h)."""
    e1, e2 = _engine(1, 0, unet_sd), _engine(2, 0, unet_sd)
    cases = [("entry", [(B, 15, 29)], 0, 0), ("enc1.2", [(B, 15, 29, 32)], 0, 0), ("enc2.2", [(B, 15, 29, 64)], 0, 0),
             ("dec6.1", [(B, 15, 29, 32)] * 2, 0, 0), ("enc3.1", [(B, 16, 31, 64)], 0, 1), ("dec2.1", [(B, 4, 7, 384)] * 2, 0, 0),
             ("dec3.up", [(B, 5, 17, 384)], 0, 0), ("dec1.up", [(B, 1, 1, 384)], 0, 0), ("dec4.up", [(B, 2, 3, 256)], 1, 0)]
    seen = set()
    for i, (piece, shapes, arg, sc) in enumerate(cases):
        xs = [_src(s, 400 + 7 * i + k) for k, s in enumerate(shapes)]
        (y1,), h1, l1 = e1.op_unet_piece(piece, xs, arg=arg, short_clip=sc)
        (y2,), h2, l2 = e2.op_unet_piece(piece, xs, arg=arg, short_clip=sc)
        assert l1 == l2 and torch.isfinite(y1).all() and torch.equal(y1, y2), (piece, l1, l2)
        assert (h1 is None) == (h2 is None) and (h1 is None or torch.equal(h1[1], h2[1])), piece
        seen.update(_families(l1))
    assert seen == {"k_resblock_in1", "k_block2d32", "k_resblock", "k_resblock_two_src", "k_conv", "k_conv_phased"}, seen


# ---------------------------------------------------------------------------------------------------------------------------------
# the small kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C", [(2, 3, 32), (4, 7, 384), (5, 6, 64), (64, 127, 32)])
def test_pool(engine, H, W, C):
    """F.avg_pool2d(2) with floor semantics on odd and even extents: ((a + b) + c) + d in fp32 is three roundings of partial sums no
    larger than |a| + |b| + |c| + |d| (the 0.25 is exact)."""
    _pool_case(engine, H, W, C)


def _pool_case(engine, H, W, C, model=MODEL_UNET_MEL, run=None):
    x = _src((B, H, W, C), 500 + H)
    (y,), _, launches = (run or engine.op_unet_piece)("pool", [x], arg=C, model=model)
    assert y.shape == (B, H // 2, W // 2, C) and _families(launches) == ["small"]
    ref = F.avg_pool2d(nchw(x).double(), 2)
    _check(nchw(y.cpu()), ref, 3 * U32 * F.avg_pool2d(nchw(x).double().abs(), 2) + 2.0 ** -149, ("pool", H, W, C))


# log10f is within 2 ulp of the true logarithm (the device library's stated accuracy); the float64 reference adds none: 3 ulp <= 6 u32 |ref|
def _log_bar(ref):
    return 6 * U32 * ref.abs() + 2.0 ** -149


@pytest.mark.parametrize("negative", [False, True], ids=["clean", "negative-input"])
def test_prep_logmel(engine, negative):
    """to_log + time padding + last-bin drop, T < Tpad, with and without per-clip frame counts: the rows past a clip's frames are
    exactly zero, and the negative-input flag is raised exactly when a value of the input (bin 127 included) is negative."""
    from voicefixer_main_amd import _lib
    engine.take_flags()
    for T, lens in ((70, None), (70, [70, 33]), (1, None), (64, [1, 64])):
        rng = np.random.default_rng(T)
        mel = torch.from_numpy((10.0 ** (rng.normal(size=(B, T, 128)) * 1.2 - 2.5)).astype(np.float32))
        mel[0, 0, 5] = 0.0          # the 1e-8 clamp
        if negative:
            mel[B - 1, T - 1, 127] = -1e-3   # the dropped bin, seen by the check only
        Tpad = (T + 63) // 64 * 64
        (x,), _, launches = engine.op_unet_piece("prep_logmel", [mel], lens=lens)
        flags = engine.take_flags()
        ref = R.prep_logmel(mel, Tpad, lens)
        assert x.shape == (B, Tpad, 127) and _families(launches) == ["small"]
        _check(x.cpu(), ref, _log_bar(ref), ("prep_logmel", T, lens))
        for b in range(B):
            L = T if lens is None else lens[b]
            assert (x[b, L:] == 0).all(), ("padded rows", T, lens, b)
        seen = negative and (lens is None or lens[B - 1] >= T)   # (a row past the clip's frames is not looked at)
        assert bool(flags & _lib.FLAG_NEGATIVE_INPUT) == seen, (T, lens, flags)


def test_prep_spec(engine):
    """(B, T, 1025) -> (B, Tpad, 1024): a copy without the last bin, zeros past each clip's frames."""
    for T, lens in ((70, None), (70, [70, 33]), (1, None)):
        _prep_spec_case(engine, T, lens)


def _prep_spec_case(engine, T, lens, model=MODEL_UNET_MEL):
    sp = _rand((B, T, 1025), 600 + T).abs()
    Tpad = (T + 63) // 64 * 64
    (x,), _, launches = engine.op_unet_piece("prep_spec", [sp], lens=lens, model=model)
    ref = torch.zeros((B, Tpad, 1024))
    for b in range(B):
        L = T if lens is None else lens[b]
        ref[b, :L] = sp[b, :L, :1024]
    assert torch.equal(x.cpu(), ref), (T, lens)
    return _families(launches)


@pytest.mark.parametrize("T", [1, 70])
def test_final_mel(engine, unet_sd, T):
    """after_conv2 + the recovered last bin + to_log(mel), rows < T of a padded trunk output: 32 products and the bias in fp32 (the bound
    with n = 32, the log term as the residual) plus log10f's own error; bin 127 is to_log(mel) alone."""
    Tpad = (T + 63) // 64 * 64
    y = _src((B, Tpad, 127, 32), 700 + T)
    rng = np.random.default_rng(T)
    mel = torch.from_numpy((10.0 ** (rng.normal(size=(B, T, 128)) * 1.2 - 2.5)).astype(np.float32))
    (out,), _, launches = engine.op_unet_piece("final", [y, mel], arg=0)
    r = R.final_mel(unet_sd, y, mel, T)
    assert out.shape == (B, T, 128) and _families(launches) == ["small"]
    _check(out.cpu(), r["ref"], (32 + 2) * U32 * (r["S"] + r["log"].abs()) + _log_bar(r["log"]), ("final", T))
    _check(out.cpu()[..., 127], r["log"][..., 127], _log_bar(r["log"][..., 127]), ("final, bin 127", T))


def test_final_spec(engine, unet_sd):
    """The spectrogram model's epilogue (mode 1) on a narrow trunk: mag = after_conv2(y), re = mag cos, im = mag sin, last bin 0."""
    _final_spec_case(engine, unet_sd, 3, 40)


def _final_spec_case(engine, sd, T, W, model=MODEL_UNET_MEL, run=None):
    """Rows >= T of the padded trunk hold NaN: a finite output read rows < T only."""
    Tpad = (T + 63) // 64 * 64
    y = _src((B, Tpad, W, 32), 800)
    y[:, T:] = float("nan")
    cos, sin = _rand((B, T, W + 1), 801), _rand((B, T, W + 1), 802)
    (re, im), _, launches = (run or engine.op_unet_piece)("final", [y, cos, sin], arg=1, model=model)
    r = R.final_spec_mag(sd, y, T)
    assert re.shape == im.shape == (B, T, W + 1)
    for got, aux, name in ((re, cos, "re"), (im, sin, "im")):
        _check(got.cpu(), r["ref"] * aux.double(), (32 + 3) * U32 * r["S"] * aux.double().abs() + 2.0 ** -149, ("final spec", name, T, W))
        assert (got[..., W] == 0).all(), name
    return _families(launches)


# ---------------------------------------------------------------------------------------------------------------------------------
# the spectrogram model's geometry: trunk width 1024, pruned (even-width) upsamplers, the two-output epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
# Level l runs at (Tpad >> (l - 1), 1024 >> (l - 1)), the bottleneck at (1, 16) and (2, 16): every level tiles exactly in W (128 tiles
# across at level 1), and plan_conv picks tile shapes no mel case gets (4 x 16, 2 x 32, 2 x 16, 1 x 128 with dead columns).  The shapes
# are resunet_pieces_f64's SPEC_* lists, read off plan_chains.unet_geometry(MODEL_UNET_SPEC, 64 | 128); the references and the
# per-element bound are the mel cases'.  B = 1 at (64, 1024) keeps the float64 convolutions of a case under a second each.
@pytest.fixture(scope="module")
def spec_sd():
    from voicefixer_main_amd import synth
    return synth.make_resunet_state_dict(2)


@pytest.fixture(scope="module")
def spec_engines(spec_sd):
    """get(precision, tuning = 0): a handle with the spectrogram ResUNet's synthetic weights (those of test_gpu_plan_chains)."""
    engines = {}

    def get(precision, tuning=0):
        if (precision, tuning) not in engines:
            engines[precision, tuning] = _engine(precision, tuning, spec_sd, MODEL_UNET_SPEC)
        return engines[precision, tuning]
    yield get
    for eng in engines.values():
        eng.close()


def test_spec_entry_block(engine, spec_engines, spec_sd):
    """The entry block at (64, 1024): the fused IN1 launch, or k_conv_c1 + k_conv in fp32."""
    eng = spec_engines(engine.precision)
    p, _ = _mode(eng)
    (H, W), = R.SPEC_FUSED_SHAPES
    assert _entry_case(eng, spec_sd, H, W, MODEL_UNET_SPEC, B=1) == (["k_resblock_in1"] if p == 1 else ["small", "k_conv"])


@pytest.mark.parametrize("piece,hw,batch", R.SPEC_FUSED_CASES, ids=[c[0] for c in R.SPEC_FUSED_CASES])
def test_spec_fused_block(engine, spec_engines, spec_sd, piece, hw, batch):
    """Level 1 at (64, 1024) -- the C = 32 identity blocks on k_block2d32, dec6.1's two sources with shortcut segments on k_resblock
    SC2 -- and the C = 64 identity blocks at (32, 512) on k_resblock G2; in fp32 each is two k_conv launches."""
    eng = spec_engines(engine.precision)
    p, _ = _mode(eng)
    (launches,) = _block_case(eng, spec_sd, piece, hw[0], hw[1], 900, model=MODEL_UNET_SPEC, B=batch)
    want = {"dec6.1": ["k_resblock_two_src"], "enc2.2": ["k_resblock"], "dec5.2": ["k_resblock"]}.get(piece, ["k_block2d32"])
    assert _families(launches) == (["k_conv", "k_conv"] if p == 0 else want), (piece, hw, launches)


def test_spec_level1_block_on_16x16_tiles(spec_engines, spec_sd):
    """VFX_TUNE_OLD_BLOCK2D at (64, 1024): the C = 32 identity block on k_resblock's 16 x 16 h tiles."""
    from voicefixer_main_amd import _lib
    piece, (H, W), batch = R.SPEC_OLD_BLOCK2D_CASE
    (launches,) = _block_case(spec_engines(1, _lib.TUNE_OLD_BLOCK2D), spec_sd, piece, H, W, 910, model=MODEL_UNET_SPEC, B=batch)
    assert _families(launches) == ["k_resblock"], launches


@pytest.mark.parametrize("piece", sorted(R.SPEC_DEEP_CASES))
def test_spec_two_launch_block(engine, spec_engines, spec_sd, piece):
    """Every deep block at its spectrogram level shapes for Tpad = 64 and 128 with short_clip 1, 0 and -2, whatever ksplit and tile
    shape the planner picks there."""
    eng = spec_engines(engine.precision)
    for i, (H, W) in enumerate(R.SPEC_DEEP_CASES[piece]):
        for launches in _block_case(eng, spec_sd, piece, H, W, 920 + i, short_clips=R.SHORT_CLIPS, model=MODEL_UNET_SPEC):
            assert _families(launches) == ["k_conv", "k_conv"] and launches[0]["out_act"] and not launches[1]["out_act"], (piece, H, W, launches)


SPEC_SPLIT_K = {1, 2, 4, 8}   # what the planner reaches over SPEC_DEEP_CASES x SHORT_CLIPS: every factor it has


def test_spec_deep_cases_split_k(engine):
    """The spectrogram cases above run ksplit 1, 2, 4 and 8 -- the planner's whole set, as the mel cases do -- each with an activated
    output and with shortcut segments plus bias, on this handle's precision and tuning."""
    act, shortcut = R.splitk_coverage(lambda piece, H, W, sc: engine.plan_unet_piece(piece, B, H, W, short_clip=sc, precision=engine.cfg.precision,
                                                                                     tuning=engine.cfg.tuning), R.SPEC_DEEP_CASES)
    assert act == SPEC_SPLIT_K and shortcut == SPEC_SPLIT_K, (act, shortcut)


@pytest.mark.parametrize("d", sorted(R.SPEC_UP_CASES))
def test_spec_upsampler(engine, spec_engines, spec_sd, d):
    """Every decoder's pruned-width ConvTranspose2d at the input shape the spectrogram chain gives it, (1, 16) -> (2, 32) up to
    (32, 512) -> (64, 1024): one row of input is the four-parity fallback, the others one launch of four phases."""
    H, W = R.SPEC_UP_CASES[d]
    assert _up_case(spec_engines(engine.precision), spec_sd, d, H, W, True, 930 + d, MODEL_UNET_SPEC) == (["k_conv"] * 4 if H == 1 else ["k_conv_phased"])


def test_spec_upsampler_odd_width(engine, spec_engines, spec_sd):
    """The unpruned width at a wide shape: (16, 256) -> (32, 513)."""
    d, (H, W) = R.SPEC_UP_WIDE_UNPRUNED
    assert _up_case(spec_engines(engine.precision), spec_sd, d, H, W, False, 940, MODEL_UNET_SPEC) == ["k_conv_phased"]


@pytest.mark.parametrize("H,W,C", R.SPEC_POOL_CASES)
def test_spec_pool(engine, spec_engines, H, W, C):
    _pool_case(spec_engines(engine.precision), H, W, C, MODEL_UNET_SPEC)


@pytest.mark.parametrize("T", R.SPEC_FINAL_T)
def test_spec_final(engine, spec_engines, spec_sd, T):
    """The two-output epilogue at W = 1024 on rows < T of a Tpad = 64 and of a Tpad = 128 trunk; the last bin exactly 0."""
    assert _final_spec_case(spec_engines(engine.precision), spec_sd, T, R.SPEC_W0, MODEL_UNET_SPEC) == ["small"]


def test_spec_prep_spec(engine, spec_engines):
    """T = 130 (Tpad = 192) with per-clip frame counts."""
    T, lens = R.SPEC_PREP_CASE
    assert _prep_spec_case(spec_engines(engine.precision), T, lens, MODEL_UNET_SPEC) == ["small"]
