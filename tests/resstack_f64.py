"""Shared by tests/test_resstack_f64_host.py and tests/test_gpu_resstack_launches.py: the float64 reference of one fused ResStack launch
of the vocoder (a layer, or a layer pair) on the operands the kernel multiplies, and the per-element bound a launch is held to.  A
plain helper module in the style of launch_parity_f64.py (whose operand forms and bounds it reuses); no tests.

One layer, on ONE clip's own positions [0, Tb) (zeros outside, as in the clip's batch-of-one call), mode p (1 split-bf16, 2 16-bit):

    a  = operand_p(LeakyReLU32(trunk))            conv1's source; the wide layer (asrc) reads the given fp16 xa = fp16(LeakyReLU32(x))
    h  = conv1_f64(a, operand_p(w1)) + b1         k3, dilation d, zero padding
    g  = LeakyReLU64(h)                           unrounded; zero outside [0, Tb) -- h IS zero there, not LeakyReLU(b1)
    y  = res + conv2_f64(g, operand_p(w2)) + b2   k3;  res = the trunk value the kernel adds: the fp32 x, fp16(x) widened (fp16 trunk),
                                                  or min(v, v * fp32(1 / slope)), v = xa (wide layer on the fp16 trunk)
    ya = LeakyReLU64(y, act_slope)

The bound.  u32 = 2^-24, f = products per operand product (3 in split-bf16), S1 = conv(|a| + da, |w1q|):

    e1 = conv(da, |w1q|) + (3 C f + 2) u32 (S1 + |b1|)  [+ 2^-17 S1, the omitted lo * lo]       |h' - h| <= e1

(launch_parity_f64._bar with n = 3 C, uncapped; da = what separates the kernel's source operand from a, see below).  The kernel
multiplies operand_p(LeakyReLU32(h')) instead of g.  LeakyReLU is 1-Lipschitz (slope <= 1), its fp32 form rounds the product once and
the slope once (4 u32 |g| covers both with room), the operand form rounds once more: r_2(v) = half an fp16 ulp of v (2^-25 in the
subnormal range), r_1(v) = 2^-17 v, r_0 = 0.  So

    dg = e1 + 4 u32 |g| + r_p(|g| + e1),   dg = 0 outside [0, Tb)
    e2 = conv(dg, |w2q|) + (3 C f + 3) u32 (conv(|g| + dg, |w2q|) + |b2| + |res| + dres) + dres  [+ 2^-17 conv(|g| + dg, |w2q|)]

Two constants the kernels' code adds (conv_common.h), derived here and never fitted:
  * The 16-bit kernels resblock_rw / resblock_r128 / resblock_w64 activate h AFTER the conversion, on the packed halves
    (lrelu_f16x2: max(q, q * s16), q = fp16(h'), s16 = fp16(slope), the product rounded to fp16).  Where h' may be negative
    (h - e1 < 0) that is two more roundings: q's, scaled by the slope, and the slope's own:
        dg += s16 * r_2(|h| + e1) + |s16 - slope| * (|h| + e1)
    k_resblock's 16-bit form rounds once (fp32 LeakyReLU, then fp16); the bound covers both forms.
  * On the fp16 trunk resblock_rw / resblock_r128 form conv1's source the same way (f16x4_lrelu): a' = max(x16, fp16(x16 * s16)), both
    factors fp16, so a' is known EXACTLY.  da = |a' - a|: the distance of the two forms, element by element (0 or one fp16 ulp, on
    negative trunk values only).  Everywhere else da = 0 in a single layer.

A pair runs two layers; the first one's output stays fp32 in registers, so its e2 is the perturbation of the second layer's input:
res = y1 with dres = e2(1), a = LeakyReLU64(y1) unrounded with da = dact(y1, e2(1)) (the same form as dg).

Stored forms: an fp16 y adds r_2(|y| + e2); ya is _act_bar's bound (the raw bound through the activation, its fp32 rounding, half an
fp16 ulp).  The bar is never looser than today's tol['conv'] * max(1, max |ref|) (twice that for a pair)."""
import numpy as np
import torch
import torch.nn.functional as F

from launch_parity_f64 import U32, _act32, _act64, _act_bar, _bar, _operand

INF = float("inf")


def conv64(a, w, d):
    """a (T, Cin), w (Cout, Cin, 3) float64 -> (T, Cout): k3, dilation d, zero padding."""
    return F.conv1d(a.T[None], w, None, padding=d, dilation=d)[0].T


def r_p(v, p):
    """The rounding of a value of magnitude <= v to the operand form of mode p."""
    if p == 2:
        e = torch.floor(torch.log2(torch.clamp(v, min=2.0 ** -24)))
        return 0.5 * 2.0 ** (torch.clamp(e, min=-14.0) - 10.0)
    if p == 1:
        return 2.0 ** -17 * v
    return torch.zeros_like(v)


def s16_of(slope):
    return float(torch.tensor(slope, dtype=torch.float32).half())


def lrelu_packed16(q, slope):
    """The packed fp16 LeakyReLU of the 16-bit kernels on fp16 values q (any dtype holding them): max(q, fp16(q * fp16(slope))).  The
    product of two fp16 numbers is exact in fp32, so one rounding."""
    q = q.float()
    return torch.maximum(q, (q * s16_of(slope)).half().float())


def dact(t, e, slope, p):
    """Bound of |operand_p'(LeakyReLU(t')) - LeakyReLU64(t)| over |t' - t| <= e, either activation form of the 16-bit mode."""
    g = _act64(t, 1, slope).abs()
    d = e + 4 * U32 * g + r_p(g + e, p)
    if p == 2:
        s16 = s16_of(slope)
        neg = (t - e < 0).double()
        d = d + neg * (s16 * r_p(t.abs() + e, 2) + abs(s16 - slope) * (t.abs() + e))
    return d


F16_MAX = 65504.0


def _layer(a, da, res, dres, layer, d, slope, p, bounds=True, sat=None):
    """sat: None, or how the 16-bit kernel of the form converts h -- 'packed' (clamp to +-65504, then LeakyReLU: resblock_rw / r128 /
    w64) or 'after' (LeakyReLU, then clamp: k_resblock) -- so that g is the CLAMPED operand; h stays the value in front of it."""
    w1, b1, w2, b2 = layer
    C = a.shape[1]
    w1q, w2q = _operand(w1, p), _operand(w2, p)
    h = conv64(a, w1q, d) + b1.double()
    if sat == "packed":
        g = _act64(h.clamp(-F16_MAX, F16_MAX), 1, slope)
    else:
        g = _act64(h, 1, slope)
        if sat == "after":
            g = g.clamp(-F16_MAX, F16_MAX)
    y = res + conv64(g, w2q, 1) + b2.double()
    if not bounds:
        return dict(a=a, h=h, g=g, y=y, e1=None, e2=None)
    S1 = conv64(a.abs() + da, w1q.abs(), d)
    e1 = conv64(da, w1q.abs(), d) + _bar(h, S1, 3 * C, p, INF, extra=b1.double().abs()[None, :])[0]
    dg = dact(h, e1, slope, p)
    S2 = conv64(g.abs() + dg, w2q.abs(), 1)
    f = 3 if p == 1 else 1
    e2 = conv64(dg, w2q.abs(), 1) + (3 * C * f + 3) * U32 * (S2 + b2.double().abs()[None, :] + res.abs() + dres) + dres
    if p == 1:
        e2 = e2 + 2.0 ** -17 * S2
    return dict(a=a, h=h, g=g, y=y, e1=e1, e2=e2)


def resstack_ref(x, layers, dils, slope, act_slope, p, tol, *, x16=False, asrc=False, bounds=True, sat=None):
    """x (Tb, C) fp32: ONE clip's own positions.  layers: one or two (w1, b1, w2, b2) in torch layout; dils: their dilations.
    -> dict: y, ya (float64 references), bar_y32 / bar_y16 (y stored as fp32 / fp16), bar_ya, and the intermediates a, g, mid (a2, g2),
    h and e1 (conv1 + b1 and its bound; h2, e1_2 of a pair's second layer), e_mid (the bound of mid).
    bounds = False: the references alone (the exact-arithmetic data needs no bar).
    sat ('packed' / 'after', see _layer): the arithmetic of the 16-bit mode where a value leaves the fp16 range -- every conversion
    clamps to +-65504 (a NaN source becomes -65504: v_med3), the values in front of the conversions (x_src, h, mid, y) stay unclamped,
    y16 / ya are the stored (clamped) forms.  Without out-of-range values it changes nothing."""
    x = x.float()
    x_src = None
    if asrc:
        xa = _act32(x, 1, slope).half()
        a, da = xa.double(), torch.zeros_like(x, dtype=torch.float64)
        if x16:
            v = xa.float()
            res = torch.minimum(v, v * (np.float32(1.0) / np.float32(slope))).double()
        else:
            res = x.double()
    elif x16:
        xt = x.half().float()
        res = xt.double()
        a = _operand(_act32(xt, 1, slope), 2)
        da = (lrelu_packed16(xt, slope).double() - a).abs()
    else:
        res = x.double()
        # (p = 0, tests/test_resstack_f64_host.py: nothing rounds, the activation neither -- the oracle's layer)
        if sat:   # the value the kernel converts, then what the conversion makes of it
            x_src = _act32(x, 1, slope).double()
            a = torch.nan_to_num(_act32(x, 1, slope), nan=-F16_MAX).clamp(-F16_MAX, F16_MAX).half().double()
        else:
            a = _operand(_act32(x, 1, slope), p) if p else _act64(x.double(), 1, slope)
        da = torch.zeros_like(a)
    L = _layer(a, da, res, torch.zeros_like(res), layers[0], dils[0], slope, p, bounds, sat)
    out = dict(a=L["a"], g=L["g"], mid=None, slope=slope, x_src=x_src, h=L["h"], e1=L["e1"], h2=None)
    if len(layers) == 2:
        y1, e_y1 = L["y"], L["e2"]
        a2 = _act64(y1, 1, slope)   # unrounded, as g: the kernel's operand lies within dact(y1, e2(1)) of it
        if sat:
            a2 = a2.clamp(-F16_MAX, F16_MAX)
        L2 = _layer(a2, dact(y1, e_y1, slope, p) if bounds else None, y1, e_y1, layers[1], dils[1], slope, p, bounds, sat)
        out.update(mid=y1, e_mid=e_y1, a2=a2, g2=L2["g"], h2=L2["h"], e1_2=L2["e1"])
        L = L2
    yf = L["y"][torch.isfinite(L["y"])]
    out.update(y=L["y"], e2=L["e2"], sat=sat, cap=(2.0 if len(layers) == 2 else 1.0) * tol * max(1.0, float(yf.abs().max()) if yf.numel() else 1.0))
    return with_act_slope(out, act_slope)


def with_act_slope(ref, act_slope):
    """The activated reference and the bars of a reference computed by resstack_ref, for another act_slope."""
    out = dict(ref)
    y, e2, cap = ref["y"], ref["e2"], ref["cap"]
    out["ya"] = ya = _act64(y, 1, act_slope)
    if ref.get("sat"):   # the stored forms of out-of-range values
        out["ya"] = ya = ya.clamp(-F16_MAX, F16_MAX)
        out["y16"] = y.clamp(-F16_MAX, F16_MAX)
    if e2 is not None:
        capt = torch.full_like(y, cap)
        out.update(bar_y32=torch.minimum(e2, capt), bar_y16=torch.minimum(e2 + r_p(y.abs() + e2, 2), capt),
                   bar_ya=_act_bar(ya, e2, act_slope, 2, cap))
    return out


def oracle_layers(x, layers, dils, slope):
    """oracle.vocoder's ResStack on x (Tb, C) float64 with these layers: the unrounded float64 layer(s)."""
    from dataclasses import replace
    from oracle import vocoder as voc
    sd = {}
    for i, (w1, b1, w2, b2) in enumerate(layers):
        sd.update({"s.res_layers.%d.1.weight" % i: w1.double(), "s.res_layers.%d.1.bias" % i: b1.double(),
                   "s.res_layers.%d.3.weight" % i: w2.double(), "s.res_layers.%d.3.bias" % i: b2.double()})
    assert dils[0] == 1   # (the oracle's stack starts at dilation 1 and multiplies by dilation_base)
    cfg = replace(voc.VocoderConfig(), res_slope=slope, dilation_base=dils[1] if len(dils) > 1 else 3)
    return voc._res_stack(sd, "s", x.double().T[None], len(layers), cfg)[0].T


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def random_layer(C, seed):
    return (_randn((C, C, 3), seed, 1.0 / np.sqrt(3 * C)), _randn((C,), seed + 1, 0.1), _randn((C, C, 3), seed + 2, 1.0 / np.sqrt(3 * C)),
            _randn((C,), seed + 3, 0.1))


def random_trunk(B, T, C, seed):
    """Random reals with negative values on a stride of positions and channels: both LeakyReLU branches occur at every seam."""
    x = _randn((B, T, C), seed)
    x[:, ::2, 1::3] = -x[:, ::2, 1::3].abs()
    x[:, 1::2, ::5] = -x[:, 1::2, ::5].abs()
    return x


EXACT_ROW_SINGLE, EXACT_ROW_PAIR = 8, 3   # nonzero weights per output channel: checked by exact_fits for every shape the tests use


def exact_layer(C, seed, per_row=2):
    """Weights in {-1, 0, 1} with `per_row` nonzero entries per output channel and convolution, biases multiples of 0.5 in [-1, 1]: with
    integer x in [-4, 4], slope 0.5 and act_slope 0.25 every intermediate of a layer or a pair is a small multiple of 2^-7 (see
    exact_fits), so every sum is exact in fp16, in the bf16 pair and in fp32, whatever the order."""
    g = torch.Generator().manual_seed(seed)

    def w():
        t = torch.zeros(C, C * 3)
        for o in range(C):
            idx = torch.randperm(C * 3, generator=g)[:per_row]
            t[o, idx] = (torch.randint(0, 2, (per_row,), generator=g) * 2 - 1).float()
        return t.reshape(C, C, 3)

    def b():
        return torch.randint(-2, 3, (C,), generator=g).float() * 0.5
    return (w(), b(), w(), b())


def exact_trunk(B, T, C, seed):
    return torch.randint(-4, 5, (B, T, C), generator=torch.Generator().manual_seed(seed)).float()


def exact_fits(ref):
    """Every reference intermediate survives .half() unchanged (then no operand, product or partial sum rounds in any mode)."""
    for k in ("a", "g", "mid", "a2", "g2", "y", "ya"):
        t = ref.get(k)
        if t is not None and not torch.equal(t.float().half().double(), t):
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------------------
# a torch emulation of the kernel (tests/test_resstack_f64_host.py): operands rounded as the mode does, fp32 accumulation, h rounded to
# the operand form, zeros past the clip's end -- with the defects that test plants
# ---------------------------------------------------------------------------------------------------------------------------------
def _conv32(a_parts, w_parts, d, drop=None):
    """fp32 convolution of operand parts: split-bf16 hi * hi + hi * lo + lo * hi, otherwise one product.  drop = (t, k): tap k of
    output position t is left out."""
    def c(a, w):
        y = F.conv1d(a.T[None], w, None, padding=d, dilation=d)[0].T
        if drop is not None:
            t, k = drop
            src = t + (k - 1) * d
            if 0 <= src < a.shape[0]:
                y = y.clone()
                y[t] -= w[:, :, k] @ a[src]
        return y
    if len(a_parts) == 2:
        (ah, al), (wh, wl) = a_parts, w_parts
        return c(al, wh) + c(ah, wl) + c(ah, wh)
    return c(a_parts[0], w_parts[0])


def _f16sat(t):
    """The kernels' conversion (conv_common.h: pack_f16x2): clamp to +-65504 -- a NaN becomes -65504 -- then round."""
    return torch.nan_to_num(t.float(), nan=-F16_MAX).clamp(-F16_MAX, F16_MAX).half()


def _parts(t, p):
    t = t.float()
    if p == 2:
        return (_f16sat(t).float(),)
    hi = t.bfloat16().float()
    return (hi, (t - hi).bfloat16().float())


def emulate(xrow, Tb, layers, dils, slope, act_slope, p, *, x16=False, asrc=False, packed=False, defect=None, where=None, record=False,
            want_raw=True, want_act=True):
    """xrow (T, C) fp32: a clip's row of the batch tensor, whatever lies past Tb included.  -> (y, ya) fp32 (Tb, C): y in its stored form
    (fp16 values on the fp16 trunk), ya = fp16(LeakyReLU32(y unrounded, act_slope)).  packed: the packed fp16 activations of
    resblock_rw / r128 / w64.  defect: None or one of DEFECTS; drop_tap drops tap 0 of conv2 at output position `where`.

    record = True: -> (y, ya, rec), rec = {site: bool}, the saturation record of every conversion site of the 16-bit mode (X, H, MID, H2,
    Y, YA: tests/f16_flag_ref.py) by the kernels' rule -- mask the positions that do not count (past the clip's end), then record
    !(|v| <= 65504) -- with the defects of FLAG_DEFECTS: 'record_before_mask' records every position of the row, computed from
    whatever the row holds past the clip's end (the outputs are the healthy ones); 'site_silent:<site>' never reports that site;
    'record_ignores_nan' writes the predicate as |v| > 65504.  want_raw / want_act: the outputs the launch stores (a site of an
    output that is not stored converts nothing)."""
    if defect == "record_before_mask":
        y, ya, _ = _emulate(xrow, Tb, layers, dils, slope, act_slope, p, x16, asrc, packed, None, where, want_raw, want_act)
        rec = _emulate(xrow, Tb, layers, dils, slope, act_slope, p, x16, asrc, packed, defect, where, want_raw, want_act)[2]
    else:
        y, ya, rec = _emulate(xrow, Tb, layers, dils, slope, act_slope, p, x16, asrc, packed, defect, where, want_raw, want_act)
    return (y, ya, rec) if record else (y, ya)


def _emulate(xrow, Tb, layers, dils, slope, act_slope, p, x16, asrc, packed, defect, where, want_raw, want_act):
    T, C = xrow.shape
    src = xrow.float().clone()
    unmasked = defect == "record_before_mask"
    if defect != "x_past_end" and not unmasked:
        src[Tb:] = 0.0            # positions past the clip's end read as zero
    inside = torch.zeros(T, 1)
    inside[:Tb] = 1.0
    if defect == "swap_pair":
        layers = (layers[1], layers[0])
    rec = {}

    def note(site, v):
        """The record of one site: v (T, C), the fp32 values in front of the conversion."""
        if p != 2 or defect == "site_silent:" + site:
            return
        if not unmasked:
            v = v[:Tb]
        bad = (v.abs() > F16_MAX) if defect == "record_ignores_nan" else ~(v.abs() <= F16_MAX)
        rec[site] = rec.get(site, False) or bool(bad.any())

    def act(t, site=None):
        if p == 2 and packed:
            if site:
                note(site, t)
            return _parts(lrelu_packed16(_f16sat(t), slope), p)
        t = _act32(t, 1, slope)
        if site:
            note(site, t)
        return _parts(t, p)

    def layer(parts, res, lay, d, site):
        w1, b1, w2, b2 = lay
        h = _conv32(parts, _parts(w1, p), d) + b1
        g = act(h, site)
        if defect == "h_bf16":
            g = (_act32(h, 1, slope).bfloat16().float(),) + ((torch.zeros_like(h),) if p == 1 else ())
        if defect == "h_past_end":   # left at LeakyReLU(b1) instead of zero
            fill = act(b1[None, :].expand(T, -1).contiguous())
            g = tuple(gp * inside + fp * (1 - inside) for gp, fp in zip(g, fill))
        elif not unmasked:
            g = tuple(gp * inside for gp in g)     # h IS zero past the clip's end
        if defect == "res_shift":
            res = torch.cat([torch.zeros(1, C), res[:-1]])
        return res + _conv32(g, _parts(w2, p), 1, (where, 0) if defect == "drop_tap" else None) + b2

    if asrc:
        xa = _f16sat(_act32(src, 1, slope)).float()   # (the producer's form: given, not converted by this launch)
        parts = (xa,)
        res = torch.minimum(xa, xa * (np.float32(1.0) / np.float32(slope))) if x16 else src
    elif x16:
        res = src.clamp(-F16_MAX, F16_MAX).half().float()   # (the producer's clamp)
        parts = _parts(lrelu_packed16(res, slope), p) if packed else _parts(_act32(res, 1, slope), p)   # fp16 in, nothing to convert
    else:
        res = src
        t = _act32(src, 1, slope)
        note("X", t)
        parts = _parts(t, p)
    y = layer(parts, res, layers[0], dils[0], "H")
    if len(layers) == 2:
        if not unmasked:
            y = y * inside           # the second layer's source and residual: the first one's output, zero past the clip's end
        t = _act32(y, 1, slope)
        note("MID", t)
        y = layer(_parts(t, p), y, layers[1], dils[1], "H2")
    if x16 and not asrc and want_raw:
        note("Y", y)
    if want_act:
        note("YA", _act32(y, 1, act_slope))
    y = y[:Tb]
    ya = _f16sat(_act32(y, 1, slope if defect == "ya_slope" else act_slope)).float()
    if x16 and not asrc:
        y = _f16sat(y).float()
    return y, ya, rec


DEFECTS = ("h_past_end", "x_past_end", "ya_slope", "drop_tap", "res_shift", "h_bf16", "swap_pair")
FLAG_DEFECTS = ("record_before_mask", "site_silent", "record_ignores_nan")

