"""Shared by the per-launch GPU parity tests (tests/test_gpu_vocoder_launches.py, tests/test_gpu_resunet_launches.py): the operand forms
of the arithmetic modes in float64 and the per-element summation bound the tests hold a launch to.  A plain helper module, no tests.

A kernel output is a sum of n products of operands a_i w_i (the source after its prologue and the weights, both rounded to the mode's
operand form), accumulated in fp32 with the bias and the residual.  Each of the n + 2 additions rounds once, so with u32 = 2^-24 and
S = sum |a_i w_i| (the float64 convolution of the |operands|)

    |y - ref| <= (n + 2) * u32 * (S + |bias| + |residual|)

where ref is the float64 sum of the same rounded operands.  Mode p: 0 fp32 (operands are the fp32 values), 1 split-bf16 (operands are
the hi + lo bf16 pair, hi = bf16(v), lo = bf16(v - hi); three MFMA products hi*hi + hi*lo + lo*hi per product, the omitted lo*lo adds
at most 2^-17 * S), 2 16-bit (operands are fp16(v))."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _operand(t, p):
    """float32 values -> the operand values the kernel multiplies, in float64."""
    t = t.float()
    if p == 2:
        return t.clamp(-65504.0, 65504.0).half().double()
    if p == 1:
        hi = t.bfloat16()
        lo = (t - hi.float()).bfloat16()
        return hi.double() + lo.double()
    return t.double()


def _act32(t, act, slope):
    t = t.float()
    if act == 2:
        return F.elu(t)
    if act == 1:
        return F.leaky_relu(t, slope)
    return t


def _act64(t, act, slope):
    if act == 2:
        return F.elu(t)
    if act == 1:
        return F.leaky_relu(t, slope)
    return t


def _products_factor(p):
    return 3 if p == 1 else 1


def _bar(ref, S, n, p, tol, extra=0.0):
    """Per-element bound of a raw fp32 output (see the module docstring); extra = |bias| + |residual|."""
    b = (n * _products_factor(p) + 2) * U32 * (S + extra)
    if p == 1:
        b = b + 2.0 ** -17 * S
    cap = tol * max(1.0, float(ref.abs().max()))
    return torch.minimum(b, torch.full_like(b, cap)), cap


def _act_bar(ref_act, bar_y, slope_max, p, cap):
    """Bound of an activated output: the raw bound through the activation (Lipschitz max(1, slope)), its fp32 rounding and the storage
    rounding of the stored form."""
    a = ref_act.abs()
    b = bar_y * max(1.0, slope_max) + 4 * U32 * a
    if p == 2:
        e = torch.floor(torch.log2(torch.clamp(a + b, min=2.0 ** -24)))
        b = b + 0.5 * 2.0 ** (torch.clamp(e, min=-14.0) - 10.0)
    elif p == 1:
        b = b + 2.0 ** -17 * (a + b)
    return torch.minimum(b, torch.full_like(b, cap))


def _check(got, ref, bar, what):
    got = got.double()
    assert torch.isfinite(got).all(), (what, "non-finite values inside the clips")
    err = (got - ref).abs()
    worst = (err / bar).max().item()
    assert worst <= 1.0, (what, "max |err| / bar = %.3g at %s (err %.3g, bar %.3g)" %
                          (worst, np.unravel_index(int((err / bar).argmax()), tuple(err.shape)), err.max().item(), bar.max().item()))
