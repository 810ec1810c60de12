"""GPU parity of the vocoder's launches, one at a time, exactly as its plan builds them (vocoder.cpp: voc_upsample_params,
voc_conv1d_params, launch_voc_final), against float64 torch on the operands the kernel sees.

The bar is derived per element from a summation bound, not taken from the mode's loose bars.  A kernel output is a sum of n products
of operands a_i w_i (the source after its prologue and the weights, both rounded to the mode's operand form), accumulated in fp32 with
the bias and the residual.  Each of the n + 2 additions rounds once, so with u32 = 2^-24 and S = sum |a_i w_i| (the float64
convolution of the |operands|)

    |y - ref| <= (n + 2) * u32 * (S + |bias| + |residual|)

where ref is the float64 sum of the same rounded operands.  Per mode:
  * fp32: operands are the fp32 values, n = taps * Cin.
  * split-bf16: operands are the hi + lo bf16 pair (rows_to_fragments / the staging code: hi = bf16(v), lo = bf16(v - hi)); each
    product is three MFMA products hi*hi + hi*lo + lo*hi, so n = 3 * taps * Cin, and the omitted lo*lo adds at most 2^-17 * S.
  * 16-bit: operands are fp16(v) (f16_rne, pack_conv modes 2 and 3; the source fp16(act(x))), n = taps * Cin.
An output stored in a 16-bit form adds its own rounding: half an fp16 ulp of the value (16-bit mode), 2^-17 relative (the hi + lo
pair), and the activation's own fp32 rounding (4 u32 relative).  The bar is never looser than TOL[p]['conv'] * max(1, max |ref|):
where the bound is above that, the mode's bar holds.  A dropped tap, a tap shifted by one position or two phases' weights swapped
change an output by the size of a whole product term, orders of magnitude above the bar.

Past the end of a clip (per-clip lengths), the kernels store nothing: k_up16's stores go through a buffer descriptor of the clip and
are dropped (upsample16.hip), and the phased k_conv launch keeps the same contract (its varlen variant returns from a tile that lies
past the clip's end and masks the stores of a straddling tile: conv.hip, VL) -- both are checked below on NaN-filled outputs.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from launch_parity_f64 import U32, _act32, _act64, _act_bar, _bar, _check, _operand, _rand   # the shared operand forms and bounds

pytestmark = pytest.mark.gpu

RES_SLOPE, UP_SLOPE = 0.01, 0.2


# ---------------------------------------------------------------------------------------------------------------------------------
# upsamplers
# ---------------------------------------------------------------------------------------------------------------------------------
def _up_ref(x, w, b, s, p, src_act):
    """(B, T, Cin) fp32 -> float64 (ref, S) of ConvTranspose1d(k = 2s, stride s) on the kernel's operands, channels-last."""
    pad, opad = s // 2 + s % 2, s % 2
    a = _operand(_act32(x, 1, UP_SLOPE), p).permute(0, 2, 1)  # the prologue or the producer applied LeakyReLU(up_slope)
    wq = _operand(w, p)
    ref = F.conv_transpose1d(a, wq, b.double(), stride=s, padding=pad, output_padding=opad)
    S = F.conv_transpose1d(a.abs(), wq.abs(), None, stride=s, padding=pad, output_padding=opad)
    return ref.permute(0, 2, 1), S.permute(0, 2, 1)


def _lens_for(B, T):
    if B == 1:
        return None
    # clips that end inside a tile of 128 positions, one of them a single position
    return [T, max(1, T - 1 - (T // 3)), 1][:B]


def _run_upsample(eng, p, Cin, s, T, B, seed, src_act, form, lens, run=None):
    """form: 'raw' fp32 y, 'act' y activated with res_slope (beside raw unless the trunk is fp16), 'trunk' the fp16 trunk (slope 1)."""
    Cout = Cin // 2
    x = _rand((B, T, Cin), seed)
    x[:, ::3, ::2] = -x[:, ::3, ::2].abs()      # negative inputs: the LeakyReLU branch of the prologue / activated source
    w = _rand((Cin, Cout, 2 * s), seed + 1, 1.0 / np.sqrt(2 * Cin))
    b = _rand((Cout,), seed + 2, 0.1)
    want_raw = form in ("raw", "act+raw")
    act_slope = {"raw": None, "act": RES_SLOPE, "act+raw": RES_SLOPE, "trunk": 1.0}[form]
    eng.take_flags()
    y, ya, up16 = (run or eng.op_voc_upsample)(x, w.numpy(), b.numpy(), s, UP_SLOPE, src_act=src_act, want_raw=want_raw, act_slope=act_slope,
                                      lens=lens)
    assert eng.take_flags() == 0, ("a device flag was raised on O(1) data", Cin, s, T, B)
    tol = eng.tol['conv']
    n = 2 * Cin
    for b_ in range(B):
        Lin = T if lens is None else lens[b_]
        L = Lin * s
        r, Sb = _up_ref(x[b_:b_ + 1, :Lin], w, b, s, p, src_act)   # the clip alone: zeros past its end
        r, Sb = r[0], Sb[0]
        bar, cap = _bar(r, Sb, n, p, tol, extra=b.double().abs()[None, :])
        if y is not None:
            _check(y[b_, :L].cpu(), r, bar, ("raw", Cin, s, T, b_))
            assert torch.isnan(y[b_, L:]).all(), ("raw output written past the clip's end", Cin, s, T, b_)
        if ya is not None:
            ra = _act64(r, 1, act_slope)
            _check(ya[b_, :L].cpu(), ra, _act_bar(ra, bar, 1.0, p, cap * max(1.0, act_slope)), ("act", Cin, s, T, b_))
            assert torch.isnan(ya[b_, L:]).all(), ("activated output written past the clip's end", Cin, s, T, b_)
    return up16


UP_T = (1, 2, 3, 127, 128, 129, 255, 257)


@pytest.mark.parametrize("Cin", [128, 256, 512, 1024, 64])
@pytest.mark.parametrize("s", [2, 3, 4, 5, 7, 9])
def test_upsampler_vs_fp64(engine, Cin, s):
    """One upsampler per (Cin, stride) over T in UP_T (around k_up16's 128-position tile), B = 1 and B = 3 with per-clip lengths that
    end inside a tile (one clip of a single position); the output form the plan gives the stage: the fp16 trunk (16-bit mode,
    Cin = 128 / 256), activated for the next convolution (Cin = 512 / 1024, raw beside it outside the 16-bit mode), raw fp32 with the
    LeakyReLU prologue in the launch (64 -> 32: the raw path of a 32-channel stack).  Every row must have run on the kernel the plan picks
    (k_up16 exactly for the 16-bit mode at Cin = 128 / 256)."""
    p = {"fp32": 0, "split-bf16": 1, "fp16-vocoder": 2}[engine.tol['name']]
    if Cin == 64:
        form, src_act = "raw", p == 2   # (the 16-bit plan reads the activated fp16 form of a 64-channel trunk; the others the raw one)
    elif Cin in (128, 256):
        form, src_act = ("trunk" if p == 2 else "act+raw"), True
    else:
        form, src_act = ("act" if p == 2 else "act+raw"), True
    Ts = UP_T if Cin <= 256 else (1, 3, 128, 129, 257)
    for i, T in enumerate(Ts):
        for B in (1, 3):
            up16 = _run_upsample(engine, p, Cin, s, T, B, 1000 * s + 10 * i + B, src_act, form, _lens_for(B, T))
            assert up16 == (p == 2 and Cin in (128, 256)), ("kernel", Cin, s, T, B, up16)


def test_upsampler_product_length_x3(engine):
    """The x3 stage of a 1.5 s clip at B = 2 (256 -> 128 channels over 7546 positions: the recalled table's third upsampler), the
    second clip ending inside a tile."""
    p = {"fp32": 0, "split-bf16": 1, "fp16-vocoder": 2}[engine.tol['name']]
    up16 = _run_upsample(engine, p, 256, 3, 7546, 2, 77, True, "trunk" if p == 2 else "act+raw", [7546, 7001])
    assert up16 == (p == 2)


@pytest.mark.parametrize("Cin", [128, 256])
def test_k_up16_matches_phased_k_conv_bitwise(Cin):
    """upsample16.hip promises the phased k_conv launch's sums bit for bit: every shape k_up16 accepts, against a handle with
    VFX_TUNE_NO_FUSED_UPSAMPLERS -- whole tensors without lengths, each clip's own positions with them."""
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import Engine
    fused, phased = Engine("cuda:0", config={"precision": 2}), Engine("cuda:0", config={"precision": 2, "tuning": _lib.TUNE_NO_FUSED_UPSAMPLERS})
    for s in (2, 3, 4, 5, 7, 9):
        for i, T in enumerate(UP_T):
            for B in (1, 3):
                lens = _lens_for(B, T)
                x = _rand((B, T, Cin), 5000 + 10 * s + i)
                w = _rand((Cin, Cin // 2, 2 * s), 6000 + s, 1.0 / np.sqrt(2 * Cin))
                b = _rand((Cin // 2,), 7000 + s, 0.1)
                _, ya, u1 = fused.op_voc_upsample(x, w.numpy(), b.numpy(), s, act_slope=1.0, lens=lens)
                _, yb, u2 = phased.op_voc_upsample(x, w.numpy(), b.numpy(), s, act_slope=1.0, lens=lens)
                assert u1 and not u2
                if lens is None:
                    assert torch.equal(ya, yb), (Cin, s, T)
                else:
                    for b_, L in enumerate(lens):
                        assert torch.equal(ya[b_, :L * s], yb[b_, :L * s]), (Cin, s, T, b_)


# ---------------------------------------------------------------------------------------------------------------------------------
# the conv1d builder
# ---------------------------------------------------------------------------------------------------------------------------------
def _conv_case(eng, p, Cin, Cout, T, B, K, dil, seed, *, reflect=False, src_act=False, act=0, slope=1.0, residual=False,
               residual_act=False, want_raw=True, next_act=0, next_slope=1.0, lens=None, run=None):
    x = _rand((B, T, Cin), seed)
    w = _rand((Cout, Cin, K), seed + 1, 1.0 / np.sqrt(K * Cin))
    b = _rand((Cout,), seed + 2, 0.1)
    res = _rand((B, T, Cout), seed + 3) if residual else None
    if res is not None:
        res[:, ::2, 1::3] = -res[:, ::2, 1::3].abs()   # negative trunk values: the inverted LeakyReLU branch
    eng.take_flags()
    y, ya = (run or eng.op_voc_conv1d)(x, w.numpy(), b.numpy(), dil=dil, reflect=reflect, src_act=src_act, act=act, slope=slope, residual=res,
                              residual_act=residual_act, want_raw=want_raw, next_act=next_act, next_slope=next_slope, lens=lens)
    assert eng.take_flags() == 0, ("a device flag was raised on O(1) data", Cin, Cout, T, K, dil)
    tol = eng.tol['conv']
    wq = _operand(w, p)
    for b_ in range(B):
        L = T if lens is None else lens[b_]
        a = _operand(_act32(x[b_:b_ + 1, :L], act, slope), p).permute(0, 2, 1)
        if reflect:
            a = F.pad(a, (K // 2, K // 2), mode="reflect")
            ref = F.conv1d(a, wq, b.double())
            S = F.conv1d(a.abs(), wq.abs())
        else:
            ref = F.conv1d(a, wq, b.double(), padding=dil * (K // 2), dilation=dil)
            S = F.conv1d(a.abs(), wq.abs(), padding=dil * (K // 2), dilation=dil)
        ref, S = ref[0].T, S[0].T
        extra = b.double().abs()[None, :]
        if res is not None:
            r = res[b_, :L]
            if residual_act:  # the residual the epilogue recovers: min(v, v * fp32(1 / res_slope)), v = fp16(LeakyReLU(r))
                v = F.leaky_relu(r, RES_SLOPE).half().float()
                r = torch.minimum(v, v * (np.float32(1.0) / np.float32(RES_SLOPE)))
            ref = ref + r.double()
            extra = extra + r.double().abs()
        bar, cap = _bar(ref, S, K * Cin, p, tol, extra=extra)
        if y is not None:
            _check(y[b_, :L].cpu(), ref, bar, ("raw", Cin, Cout, T, K, dil, b_))
            assert torch.isnan(y[b_, L:]).all(), ("raw output written past the clip's end", T, b_)
        if ya is not None:
            ra = _act64(ref, next_act, next_slope)
            _check(ya[b_, :L].cpu(), ra, _act_bar(ra, bar, next_slope, p, cap), ("act", Cin, Cout, T, K, dil, b_))
            assert torch.isnan(ya[b_, L:]).all(), ("activated output written past the clip's end", T, b_)


def _mode(engine):
    return {"fp32": 0, "split-bf16": 1, "fp16-vocoder": 2}[engine.tol['name']]


def test_condnet_layer(engine):
    """condnet layer i > 0: 512 <- the activated ELU output of the previous layer, k3, ELU into the activated form; and the first one
    (128 -> 512 on the raw conditioning); T around the 128-position tile, with and without per-clip lengths."""
    p = _mode(engine)
    for i, (T, B) in enumerate(((1, 1), (2, 1), (129, 3), (257, 1))):
        lens = _lens_for(B, T)
        _conv_case(engine, p, 128, 512, T, B, 3, 1, 100 + i, src_act=False, want_raw=False, next_act=2, lens=lens)
        _conv_case(engine, p, 512, 512, T, B, 3, 1, 200 + i, src_act=True, act=2, want_raw=False, next_act=2, lens=lens)


@pytest.mark.parametrize("T", [4, 5, 6, 7, 8, 9, 130])
def test_k7_reflect_conv(engine, T):
    """generator.1: ReflectionPad1d(3) + Conv1d k7 on ELU(condnet) (the activated ELU form), 512 -> 1024, activated with LeakyReLU(up_slope)
    for upsampler 0; T from 4 (reflect pad 3 at its shortest) to 9, and past a tile; with lengths, each clip reflects at its own end."""
    p = _mode(engine)
    lens = None if T < 6 else [T, 4, T - 1]
    _conv_case(engine, p, 512, 1024, T, 1 if lens is None else 3, 7, 1, 300 + T, reflect=True, src_act=True, act=2, want_raw=False,
               next_act=1, next_slope=UP_SLOPE, lens=lens)


@pytest.mark.parametrize("dil", [1, 3, 9, 27])
def test_c512_resstack_layer_two_launches(engine, dil):
    """A C = 512 ResStack layer as the plan runs it: conv1 (k3, dilation dil) on the activated trunk, activated for conv2; conv2 (k3)
    adds the residual -- in the 16-bit mode the activated fp16 trunk itself, inverted in the epilogue (residual_act) -- and writes the
    next trunk activated (and raw outside the 16-bit mode).  T < dilation included; the trunk has negative values."""
    p = _mode(engine)
    for i, (T, B) in enumerate(((2, 1), (dil + 1, 1), (130, 3))):
        lens = _lens_for(B, T)
        _conv_case(engine, p, 512, 512, T, B, 3, dil, 400 + 10 * dil + i, src_act=True, act=1, slope=RES_SLOPE, want_raw=False,
                   next_act=1, next_slope=RES_SLOPE, lens=lens)
        _conv_case(engine, p, 512, 512, T, B, 3, 1, 500 + 10 * dil + i, src_act=True, act=1, slope=RES_SLOPE, residual=True,
                   residual_act=(p == 2), want_raw=(p != 2), next_act=1, next_slope=RES_SLOPE, lens=lens)


def test_raw_32_channel_layer(engine):
    """The 32-channel raw form (a 32-channel stack of another layer table): raw fp32 source through the launch's LeakyReLU prologue,
    raw residual, raw output; dilations 1 and 27 (T < 27 included)."""
    p = _mode(engine)
    for i, (T, B, dil) in enumerate(((20, 1, 27), (300, 3, 1), (300, 3, 27), (1, 1, 1))):
        lens = _lens_for(B, T)
        _conv_case(engine, p, 32, 32, T, B, 3, dil, 600 + i, act=1, slope=RES_SLOPE, lens=lens)
        _conv_case(engine, p, 32, 32, T, B, 3, 1, 650 + i, act=1, slope=RES_SLOPE, residual=True, lens=lens)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tail
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_f16", [False, True], ids=["f32-trunk", "f16-trunk"])
def test_voc_final(engine, x_f16):
    """tanh(conv1d(ReflectionPad1d(3)(LeakyReLU(x, 0.2)))) to one channel on an fp32 or fp16 trunk, with and without per-clip lengths:
    each clip reflects at its own end and writes nothing past it.  The tail is plain fp32 arithmetic (n = 7 C products)."""
    for i, (B, T, C, lens) in enumerate(((1, 4, 64, None), (1, 1000, 64, None), (3, 777, 64, [777, 500, 4]), (2, 300, 128, [300, 13]))):
        _final_case(engine, B, T, C, lens, x_f16, 800 + i)


def _final_case(engine, B, T, C, lens, x_f16, seed, run=None):
    x = _rand((B, T, C), seed)
    w = _rand((1, C, 7), seed + 50, 1.0 / np.sqrt(7 * C))
    bias = 0.05
    engine.take_flags()
    wav = (run or engine.op_voc_final)(x, w.numpy(), bias, UP_SLOPE, x_f16=x_f16, lens=lens).cpu()
    assert engine.take_flags() == 0, ("a device flag was raised on O(1) data", B, T, C)
    xs = x.half().float() if x_f16 else x
    for b_ in range(B):
        L = T if lens is None else lens[b_]
        a = F.pad(F.leaky_relu(xs[b_:b_ + 1, :L].double(), UP_SLOPE).permute(0, 2, 1), (3, 3), mode="reflect")
        pre = F.conv1d(a, w.double())[0, 0] + bias
        S = F.conv1d(a.abs(), w.double().abs())[0, 0]
        ref = torch.tanh(pre)
        bar = (7 * C + 2) * U32 * (S + abs(bias)) + 8 * U32
        bar = torch.minimum(bar, torch.full_like(bar, engine.tol['conv']))
        _check(wav[b_, :L], ref, bar, ("tail", B, T, C, b_))
        assert torch.isnan(wav[b_, L:]).all(), ("tail written past the clip's end", b_)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole vocoder
# ---------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (2, 64), (1, 300)], ids=["T1", "T2", "T64", "3s"])
def test_vocoder_pointwise_vs_oracle(engine, voc_sd, B, T):
    """The whole vocoder against oracle.vocoder held to the pointwise voc_max bar at 1, 2 and 64 frames and at a 3 s clip (300 frames:
    the x3 stages span dozens of 128-position tiles)."""
    rng = np.random.default_rng(31 + T)
    mel = (10.0 ** (rng.normal(size=(B, 1, T, 128)) * 1.2 - 2.5)).astype(np.float32)
    if (B, T) not in _ORACLE:   # (one oracle run per shape for the three modes)
        from oracle import vocoder as voc
        _ORACLE[(B, T)] = voc.vocoder(voc_sd, torch.from_numpy(mel)).numpy()[:, 0]
    ref = _ORACLE[(B, T)]
    got = engine.vocoder(torch.from_numpy(mel[:, 0])).cpu().numpy()
    assert got.shape == ref.shape == (B, (T + T % 2 + 4) * 441)
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() < engine.tol['voc_max'], np.abs(got - ref).max()
