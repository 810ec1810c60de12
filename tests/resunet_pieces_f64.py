"""Float64 references of the pieces of the ResUNet plan (resunet.cpp: TrunkBuilder), one launch at a time, on the operands the launch
multiplies.  A plain helper module, no tests: tests/test_gpu_resunet_launches.py holds every launch to them, and
tests/test_resunet_pieces_host.py chains them in plan order against oracle.resunet.

Everything is torch.nn.functional in float64 on weights taken from the state_dict the handle loaded (keys as
synth.make_resunet_state_dict emits them).  Eval-mode BatchNorm is folded in float64; a source passes through its prologue (the
folded affine, LeakyReLU or ReLU) in fp32 and is then rounded to the mode's operand form (launch_parity_f64._operand).

Activations are channels-last (B, H, W, C) float32 tensors, as the plan stores them; the functions return NCHW float64 tensors:
`ref` (the float64 sum on the operands), `S` (the same convolution of the |operands|), `E` (a bound of what the launch's own fp32
prologue may differ from this module's, pushed through the |weights|; see prologue()) and `n` (taps x channels over all segments).
"""
import torch
import torch.nn.functional as F

import plan_chains as PC
from launch_parity_f64 import U32, _operand
from voicefixer_main_amd.engine import MODEL_UNET_SPEC

BN_EPS = 1e-5
SLOPE = 0.01


def block_prefix(piece):
    """Piece name of vfx_op_unet_piece -> state_dict prefix of its ConvBlockRes (or of the decoder, for "dec<d>.up")."""
    if piece == "entry":
        return "encoder_block1.conv_block1"
    if piece == "bott":
        return "conv_block7"
    if piece == "after":
        return "after_conv_block1"
    l, j = piece[3:].split(".")
    if piece.startswith("enc"):
        return "encoder_block%s.conv_block%s" % (l, j)
    return "decoder_block%s" % l if j == "up" else "decoder_block%s.conv_block%d" % (l, int(j) + 1)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def fold_bn(sd, p):
    """Eval-mode BatchNorm2d folded in float64 -> (scale, shift, |mean * scale|), each (C,)."""
    g, b, m, v = (sd[p + k].double() for k in (".weight", ".bias", ".running_mean", ".running_var"))
    scale = g / torch.sqrt(v + BN_EPS)
    return scale, b - m * scale, (m * scale).abs()


def prologue(x, bn, slope, p):
    """x (B, C, H, W) fp32 values -> (operands, err) of LeakyReLU(scale * x + shift, slope) (slope 0: ReLU), float64.

    The reference evaluates the affine exactly and rounds once to fp32.  The launch folds the BatchNorm in fp32 (the scale through an
    addition, a square root and a division: relative error 3 u32; the shift b - m * scale through two more roundings) and evaluates
    scale * x + shift with one or two roundings, so its fp32 value t differs from the reference's by at most
        u32 * (5 |x scale| + 4 |mean scale| + 3 |shift|),
    the LeakyReLU multiplies by the slope (one rounding, u32 |a|), and two fp32 values that close round to operand values at most one
    step of the operand form further apart (split-bf16: the step of the lo half, 2^-16 |a|; fp32: none)."""
    scale, shift, ms = (t[None, :, None, None] for t in bn)
    xs = x.double() * scale
    a32 = F.leaky_relu((xs + shift).float(), slope)
    op = _operand(a32, p)
    err = U32 * (5 * xs.abs() + 4 * ms + 3 * shift.abs() + a32.double().abs())
    if p == 1:
        err = err + 2.0 ** -16 * op.abs()
    return op, err


def _conv(a, w, pad):
    return F.conv2d(a, w, padding=pad)


def conv1(sd, prefix, srcs, p):
    """conv1 of a ConvBlockRes over cat(srcs): every source through bn1's slice of its channels and LeakyReLU."""
    bn = fold_bn(sd, prefix + ".bn1")
    w = _operand(sd[prefix + ".conv1.weight"], p)
    ref = S = E = 0.0
    c0 = 0
    for x in srcs:
        C = x.shape[-1]
        a, err = prologue(nchw(x), tuple(t[c0:c0 + C] for t in bn), SLOPE, p)
        ws = w[:, c0:c0 + C]
        ref = ref + _conv(a, ws, 1)
        S = S + _conv(a.abs(), ws.abs(), 1)
        E = E + _conv(err, ws.abs(), 1)
        c0 += C
    assert c0 == w.shape[1]
    return dict(ref=ref, S=S, E=E, n=9 * c0, extra=0.0)


def h_activated(sd, prefix, h):
    """LeakyReLU(bn2(h)) in float64 -- what conv1's launch stores for conv2 -- and the bound of the fp32 affine's own rounding (see
    prologue()), to be added to |scale| x the bound of h before launch_parity_f64._act_bar."""
    scale, shift, ms = (t[None, :, None, None] for t in fold_bn(sd, prefix + ".bn2"))
    hs = h * scale
    return F.leaky_relu(hs + shift, SLOPE), scale.abs(), U32 * (5 * hs.abs() + 4 * ms + 3 * shift.abs())


def conv2(sd, prefix, h_op, srcs, p, residual=None):
    """conv2 of a ConvBlockRes on the operand values h_op (B, C, H, W) float64 of its activated source, plus the block's shortcut:
    the 1x1 convolution of the raw sources with its bias where the block has one, else the raw residual (default: srcs[0])."""
    w = _operand(sd[prefix + ".conv2.weight"], p)
    ref = _conv(h_op, w, 1)
    S = _conv(h_op.abs(), w.abs(), 1)
    n = 9 * w.shape[1]
    if (prefix + ".shortcut.weight") in sd and residual is None:
        wsc = _operand(sd[prefix + ".shortcut.weight"], p)
        bias = sd[prefix + ".shortcut.bias"].double()[None, :, None, None]
        c0 = 0
        for x in srcs:
            C = x.shape[-1]
            a = _operand(nchw(x), p)
            ref = ref + _conv(a, wsc[:, c0:c0 + C], 0)
            S = S + _conv(a.abs(), wsc[:, c0:c0 + C].abs(), 0)
            c0 += C
        n += c0
        ref = ref + bias
        extra = bias.abs()
    else:
        res = nchw(srcs[0]).double() if residual is None else residual
        ref = ref + res
        extra = res.abs()
    return dict(ref=ref, S=S, E=0.0, n=n, extra=extra, w_abs=w.abs())


def entry_conv1(sd, x, p):
    """encoder_block1.conv_block1's conv1 and shortcut on the plane x (B, H, W): plain fp32 multiply-adds in every mode (nine per
    output; small_ops.hip k_conv_c1, resblock.hip IN1), so the operands are the fp32 values and every product is one product.
    -> (conv1 dict, shortcut (B, 32, H, W) float64 = wsc * x + bsc)."""
    prefix = "encoder_block1.conv_block1"
    a, err = prologue(x[:, None], fold_bn(sd, prefix + ".bn1"), SLOPE, 0)
    w = sd[prefix + ".conv1.weight"].double()
    sc = F.conv2d(x[:, None].double(), sd[prefix + ".shortcut.weight"].double(), sd[prefix + ".shortcut.bias"].double())
    return dict(ref=_conv(a, w, 1), S=_conv(a.abs(), w.abs(), 1), E=_conv(err, w.abs(), 1), n=9, extra=0.0), sc


def upsample(sd, prefix, x, prune_w, p):
    """DecoderBlockRes4B's BN -> ReLU -> ConvTranspose2d(k3, s2, p0) -> prune (time always, frequency when prune_w).  An output pixel
    sums 1, 2 or 4 taps depending on its parity: n is the largest, 4 Cin."""
    a, err = prologue(nchw(x), fold_bn(sd, prefix + ".bn1"), 0.0, p)
    w = _operand(sd[prefix + ".conv1.weight"], p)

    def up(t, wt):
        y = F.conv_transpose2d(t, wt, stride=2)[:, :, :-1]
        return y[..., :-1] if prune_w else y
    return dict(ref=up(a, w), S=up(a.abs(), w.abs()), E=up(err, w.abs()), n=4 * w.shape[0], extra=0.0)


def block_chain(sd, prefix, srcs, p):
    """One whole ConvBlockRes from the pieces above (conv2 reads the operand form of the activated h): (B, H, W, C) float32."""
    h = h_activated(sd, prefix, conv1(sd, prefix, srcs, p)["ref"])[0]
    return nhwc(conv2(sd, prefix, _operand(h.float(), p), srcs, p)["ref"]).float().contiguous()


def entry_chain(sd, x, p):
    c1, sc = entry_conv1(sd, x, p)
    prefix = "encoder_block1.conv_block1"
    h = h_activated(sd, prefix, c1["ref"])[0]
    return nhwc(conv2(sd, prefix, _operand(h.float(), p), [], p, residual=sc)["ref"]).float().contiguous()


def pool(x):
    return nhwc(F.avg_pool2d(nchw(x).double(), 2)).float().contiguous()


def prep_logmel(mel, Tpad, lens=None):
    """(B, T, 128) linear mel -> (B, Tpad, 127) float64: log10(max(mel, 1e-8)) without the last bin, zeros past each clip's frames."""
    B, T, _ = mel.shape
    out = torch.zeros((B, Tpad, 127), dtype=torch.float64)
    for b in range(B):
        L = T if lens is None else min(T, lens[b])
        out[b, :L] = torch.log10(torch.clamp(mel[b, :L, :127].double(), min=1e-8))
    return out


def final_mel(sd, y, mel, T):
    """after_conv2 (1x1, 32 -> 1, bias) + the recovered last bin + to_log(mel): y (B, Tpad, 127, 32), mel (B, T, 128) -> dict with
    ref, S (B, T, 128) float64 and the log term."""
    w = sd["after_conv2.weight"].double().reshape(32)
    v = (y[:, :T].double() * w).sum(-1) + sd["after_conv2.bias"].double()
    S = (y[:, :T].double().abs() * w.abs()).sum(-1) + sd["after_conv2.bias"].double().abs()
    lg = torch.log10(torch.clamp(mel.double(), min=1e-8))
    return dict(ref=F.pad(v, (0, 1)) + lg, S=F.pad(S, (0, 1)), log=lg)


def trunk_chain(sd, x, prune_w, p=0):
    """The trunk both ResUNets share, piece by piece in plan order: entry, encoders with pools, bottleneck, decoders (upsample, the
    two-source block, three more), after.  x (B, Tpad, W) float32 -> (B, Tpad, W, 32) float32.  prune_w: the spectrogram model's
    even-width upsamplers."""
    y = entry_chain(sd, x, p)
    skips = []
    for l in range(1, 7):
        for j in range(2 if l == 1 else 1, 5):
            y = block_chain(sd, block_prefix("enc%d.%d" % (l, j)), [y], p)
        skips.append(y)
        y = pool(y)
    y = block_chain(sd, block_prefix("bott"), [y], p)
    for d in range(1, 7):
        up = nhwc(upsample(sd, block_prefix("dec%d.up" % d), y, prune_w, p)["ref"]).float().contiguous()
        y = block_chain(sd, block_prefix("dec%d.1" % d), [up, skips[6 - d]], p)
        for j in (2, 3, 4):
            y = block_chain(sd, block_prefix("dec%d.%d" % (d, j)), [y], p)
    return block_chain(sd, block_prefix("after"), [y], p)


def generator_mel_chain(sd, mel, p=0):
    """The mel ResUNet as the plan runs it, piece by piece: prep, the trunk, final.  mel (B, T, 128) float32 -> (B, T, 128) float64."""
    B, T, _ = mel.shape
    Tpad = (T + 63) // 64 * 64
    return final_mel(sd, trunk_chain(sd, prep_logmel(mel, Tpad).float(), False, p), mel, T)["ref"]


def final_spec_mag(sd, y, T):
    """after_conv2 (1x1, 32 -> 1, bias) on rows < T of the trunk's output y (B, Tpad, W, 32), the last bin 0 -> dict with ref and S
    (B, T, W + 1) float64: the magnitude the spectrogram model's epilogue multiplies with cos and sin."""
    w = sd["after_conv2.weight"].double().reshape(32)
    bias = sd["after_conv2.bias"].double()
    mag = (y[:, :T].double() * w).sum(-1) + bias
    S = (y[:, :T].double().abs() * w.abs()).sum(-1) + bias.abs()
    return dict(ref=F.pad(mag, (0, 1)), S=F.pad(S, (0, 1)))


def prep_spec(sp, Tpad, lens=None):
    """(B, T, W + 1) magnitudes -> (B, Tpad, W) float32: a copy without the last bin, zeros past each clip's frames."""
    B, T, W1 = sp.shape
    out = torch.zeros((B, Tpad, W1 - 1))
    for b in range(B):
        L = T if lens is None else min(T, lens[b])
        out[b, :L] = sp[b, :L, :W1 - 1]
    return out


def spec_mag_chain(sd, sp, p=0):
    """The spectrogram ResUNet's magnitude as the plan runs it: prep_spec, the trunk with pruned upsamplers, after_conv2 with the last
    bin 0.  sp (B, T, 1025) float32 -> (B, T, 1025) float64."""
    B, T, _ = sp.shape
    Tpad = (T + 63) // 64 * 64
    return final_spec_mag(sd, trunk_chain(sd, prep_spec(sp, Tpad), True, p), T)["ref"]


# The deep pieces (two launches of k_conv each: C >= 128, and the blocks with a 1x1 shortcut above C = 32) at the mel net's own level shapes for Tpad = 64 and 128 --
# level l runs at (Tpad >> (l - 1), 127 >> (l - 1)), the bottleneck at (1, 1) and (2, 1) -- plus shapes that are no multiple of a tile.
def _level(l, W0=127):
    return [(64 >> (l - 1), W0 >> (l - 1)), (128 >> (l - 1), W0 >> (l - 1))]


DEEP_CASES = {
    "enc2.1": _level(2),   # (32 -> 64 with a shortcut: two launches at C = 64 too, and the one place the shortcut launch does not split)
    "enc3.1": _level(3), "enc3.2": _level(3) + [(9, 13)], "enc4.1": _level(4), "enc4.3": _level(4), "enc5.1": _level(5),
    "enc5.2": _level(5), "enc6.1": _level(6), "bott": [(1, 1), (2, 1)],
    "dec1.1": _level(6), "dec2.1": _level(5), "dec3.1": _level(4) + [(5, 9)], "dec4.1": _level(3), "dec5.1": _level(2),
}
SHORT_CLIPS = (1, 0, -2)


def splitk_coverage(plan, cases=None):
    """plan(piece, H, W, short_clip) -> launches (Engine.plan_unet_piece).  -> the ksplit values the deep cases (default: DEEP_CASES)
    run with an activated output, and with shortcut segments plus bias."""
    act, shortcut = set(), set()
    for piece, shapes in (DEEP_CASES if cases is None else cases).items():
        for H, W in shapes:
            for sc in SHORT_CLIPS:
                for l in plan(piece, H, W, sc):
                    if l["family"] == "k_conv" and l["out_act"]:
                        act.add(l["ksplit"])
                    if l["family"] == "k_conv" and l["bias"] and l["nseg"] >= 2:
                        shortcut.add(l["ksplit"])
    return act, shortcut


# ---------------------------------------------------------------------------------------------------------------------------------
# The spectrogram model's geometry: trunk width 1024, even-width (pruned) upsamplers, so level l runs at (Tpad >> (l - 1), 1024 >> (l - 1))
# and the bottleneck at (1, 16) and (2, 16).  Every shape is read off plan_chains.unet_geometry(MODEL_UNET_SPEC, T) for T = 64 and
# T = 128 -- the (H, W) the chain of the network's own pieces hands each piece -- not typed in.
# ---------------------------------------------------------------------------------------------------------------------------------
SPEC_W0 = PC.UNET_WIDTH[MODEL_UNET_SPEC]
SPEC_T = (64, 128)


def spec_shapes(piece, Ts=SPEC_T):
    """-> [(H, W)]: what the spectrogram chain hands `piece` for clips of each T in Ts frames ("pool": every level's, in order)."""
    return [(H, W) for T in Ts for pc, _, H, W in PC.unet_geometry(MODEL_UNET_SPEC, T) if pc == piece]


SPEC_FUSED_SHAPES = spec_shapes("entry", (64,))                      # level 1 at Tpad = 64: (64, 1024)
SPEC_DEEP_CASES = {piece: spec_shapes(piece) for piece in DEEP_CASES}
SPEC_UP_CASES = {d: spec_shapes("dec%d.up" % d, (64,))[0] for d in range(1, 7)}   # (1, 16) -> (2, 32) ... (32, 512) -> (64, 1024)
SPEC_UP_WIDE_UNPRUNED = (5, SPEC_UP_CASES[5])                        # the one arg = 0 case: (16, 256) -> (32, 513)
# (piece, (H, W), B): the single-launch blocks (two k_conv launches each in fp32); B = 1 at (64, 1024) keeps the float64 reference short
SPEC_FUSED_CASES = [(piece, spec_shapes(piece, (64,))[0], 1) for piece in ("enc1.2", "dec6.1", "after")] + \
                   [(piece, spec_shapes(piece, (64,))[0], 2) for piece in ("enc2.2", "dec5.2")]
SPEC_OLD_BLOCK2D_CASE = ("enc1.3", spec_shapes("enc1.3", (64,))[0], 1)
SPEC_POOL_CASES = [(64, SPEC_W0, 32), (2, SPEC_W0 >> 5, 384)]         # level 1 at Tpad = 64, level 6 at Tpad = 64
SPEC_FINAL_T = (3, 70)                                              # T < Tpad = 64, and T = 70 on a Tpad = 128 trunk
SPEC_PREP_CASE = (130, [130, 67])                                   # T, frames per clip


def spec_launch_cases(precision):
    """Every spectrogram-geometry case of tests/test_gpu_resunet_launches.py as the arguments of Engine.plan_unet_piece:
    -> [(piece, B, H, W, arg, short_clip, tuning name or None)].  tests/test_resunet_pieces_host.py holds the families these launch to
    the whole spectrogram plan's."""
    out = [("entry", 1) + SPEC_FUSED_SHAPES[0] + (0, 0, None)]
    out += [(piece, B) + hw + (0, 0, None) for piece, hw, B in SPEC_FUSED_CASES]
    if precision:
        piece, hw, B = SPEC_OLD_BLOCK2D_CASE
        out.append((piece, B) + hw + (0, 0, "TUNE_OLD_BLOCK2D"))
    out += [(piece, 2, H, W, 0, sc, None) for piece, shapes in SPEC_DEEP_CASES.items() for H, W in shapes for sc in SHORT_CLIPS]
    out += [("dec%d.up" % d, 2) + hw + (1, 0, None) for d, hw in SPEC_UP_CASES.items()]
    out.append(("dec%d.up" % SPEC_UP_WIDE_UNPRUNED[0], 2) + SPEC_UP_WIDE_UNPRUNED[1] + (0, 0, None))
    out += [("pool", 2, H, W, C, 0, None) for H, W, C in SPEC_POOL_CASES]
    out += [("final", 2, T, SPEC_W0, 1, 0, None) for T in SPEC_FINAL_T]
    out.append(("prep_spec", 2, SPEC_PREP_CASE[0], SPEC_W0 + 1, 0, 0, None))
    return out
