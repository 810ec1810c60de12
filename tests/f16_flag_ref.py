"""Shared by tests/test_f16_flag_host.py and tests/test_gpu_f16_flag_launches.py: the oracle of VFX_FLAG_F16_SATURATED for ONE launch
of the 16-bit vocoder, and the planted data that delivers a chosen value to a chosen conversion site.  A plain helper module, no tests.

The oracle models no arithmetic of its own: the values a launch converts to fp16, and their error bars, are those of the float64
references the launch tests already hold the kernels to (resstack_f64.resstack_ref with sat = the form's conversion order; the
upsampler / conv1d references of launch_parity_f64), restricted to the positions that count -- a clip's own positions [0, Tb).

Sites of a fused ResStack launch (16-bit forms only; a split-bf16 form converts nothing and has no site):
    X     fp16(LeakyReLU32(x)): an fp32 source patch staged as operands -- the forms that read a raw fp32 trunk (f32trunk-c64 / -c128,
          hionly-c64); the fp16 trunk is activated on the packed halves (nothing to convert), the wide layer reads the producer's xa
    H     conv1 + b1: in front of the packed LeakyReLU in resblock_rw / r128 / w64, behind the fp32 one in k_resblock
    MID   LeakyReLU32(y1) between the two layers of a pair (read from the kernels: the activated value is what is converted; the raw
          y1 stays fp32 in registers)
    H2    the second layer's H
    Y     the fp16 trunk output (fp16 trunk, not the wide layer, and only where the launch stores y)
    YA    fp16(LeakyReLU32(y, act_slope)), where the launch stores ya
Sites of a conv1d / upsampler launch: SRC (the launch's own prologue on a raw fp32 source) and OUT (the stored fp16 output).

Verdict of a site, and of a launch (any site raises / every site is quiet), from the code's predicates -- !(|x| <= 65504) for the
bool and bit-pattern records, "a half reached 0x7bff" for the packed sat16 record -- and the fp16 grid, nothing measured:
    must raise      some counted value has |ref| - bar >= 65520 (halfway between 65504 and 2^16: rounds past the largest fp16 in either
                    record), or is an infinity or a NaN
    must not raise  every counted value has |ref| + bar <= 65472, the largest fp16 below 65504
    undecided       otherwise (exactly 65504 is the one value on which the record types differ: sat16 raises, the others do not)
On the exact-arithmetic data (small integers, weights in {-1, 0, 1} and powers of two: every product and partial sum is a multiple of
2^-7 that fp32 holds, hence exact in any order; every operand an fp16 number: exact_sat_fits) the delivered value is known bit for
bit and the bar is zero."""
import torch

import resstack_f64 as R
from launch_parity_f64 import U32, _act64

FLAG = 2                     # voicefixer_main_amd._lib.FLAG_F16_SATURATED
RAISE, QUIET = 65520.0, 65472.0
RAISE_VALUES = (2.0 ** 17, -2.0 ** 17, 65520.0, -65520.0)
QUIET_VALUES = (65472.0, -65472.0)
PACKED = {"k_resblock": "after", "rw": "packed", "r128": "packed", "w64": "packed"}


def site_verdict(ref, bar):
    """True: must raise; False: must not raise; None: undecided."""
    ok = torch.isfinite(ref) & torch.isfinite(bar)
    if not ok.all():
        return True
    a = ref.abs()
    if ((a - bar) >= RAISE).any():
        return True
    if ((a + bar) <= QUIET).all():
        return False
    return None


def verdict(sites):
    """sites {name: (ref, bar)} -> (verdict of the launch, {name: verdict})."""
    per = {k: site_verdict(v, b) for k, (v, b) in sites.items()}
    if any(v is True for v in per.values()):
        return True, per
    if all(v is False for v in per.values()):
        return False, per
    return None, per


def exact_sat_fits(ref, y16=True, ya=True):
    """The exact-arithmetic criterion with out-of-range values in play: every operand (a, g, a2, g2: the CLAMPED forms) is an fp16
    number, and every value in front of a conversion (h, mid, h2, y) a multiple of 2^-7 that fp32 holds -- the large ones are single
    products on silent channels (plant), the rest small: no partial sum rounds in any order."""
    for k in ("a", "g", "a2", "g2"):
        t = ref.get(k)
        if t is not None and not torch.equal(t.float().half().double(), t):
            return False
    for k in ("h", "mid", "h2", "y"):
        t = ref.get(k)
        if t is not None:
            t = t[torch.isfinite(t)]
            if not (torch.equal((t * 128).round(), t * 128) and torch.equal(t.float().double(), t)):
                return False
    for k in ("y16", "ya"):   # the stored forms (y16 only where the launch stores an fp16 y)
        t = ref.get(k) if (ya if k == "ya" else y16) else None
        if t is not None:
            t = t[torch.isfinite(t)]
            if not torch.equal(t.float().half().double(), t):
                return False
    return True


def resstack_sites(ref, *, p, x16, asrc, family, pair, want_raw, want_act, act_slope, exact):
    """ref = resstack_ref(..., sat = PACKED[family]) of ONE clip -> {site: (value in front of the conversion, bar)}."""
    if p != 2:
        return {}
    slope = ref["slope"]

    def entry(v, e, lip=1.0):
        if exact:
            return v, torch.zeros_like(v)
        return v, e * lip + 4 * U32 * torch.nan_to_num(v.abs(), nan=0.0, posinf=0.0)

    def hsite(h, e):
        return entry(h if PACKED[family] == "packed" else _act64(h, 1, slope), e)

    s = {}
    if ref["x_src"] is not None and not asrc:
        s["X"] = entry(ref["x_src"], torch.zeros_like(ref["x_src"]))
    s["H"] = hsite(ref["h"], ref["e1"])
    if pair:
        s["MID"] = entry(_act64(ref["mid"], 1, slope), ref["e_mid"])
        s["H2"] = hsite(ref["h2"], ref["e1_2"])
    if x16 and not asrc and want_raw:
        s["Y"] = entry(ref["y"], ref["e2"])
    if want_act:
        s["YA"] = entry(_act64(ref["y"], 1, act_slope), ref["e2"], max(1.0, act_slope))
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# planted data: one value at one site at one (position, channel), on resstack_f64's exact-arithmetic data
# ---------------------------------------------------------------------------------------------------------------------------------
STAGE = {"H": 0, "MID": 1, "Y1": 1, "H2": 2, "Y2": 3}   # the convolution whose output the value is (Y1 / Y2: the y of a single / a pair)


def decompose(v, k=1.0):
    """k * v = gain * x0 + b with an fp16 source value x0 <= 4096, a weight gain = +-32 k (inside the weight check's [2^-14, 1024]) and
    a bias b: 65520 = 32 * 2047 + 16 is no single fp16 product.  k = 1 / slope (a power of two) delivers a negative v THROUGH a
    LeakyReLU that runs in front of the conversion."""
    s = k if v > 0 else -k
    x0, b = {2.0 ** 17: (4096.0, 0.0), 65520.0: (2047.0, 16.0), 65504.0: (2047.0, 0.0), 65472.0: (2046.0, 0.0)}[abs(v)]
    return x0, 32.0 * s, b * s


def _clone(x, layers):
    return x.clone(), [[t.clone() for t in lay] for lay in layers]


def _quiet(x, layers, chans):
    """Channels `chans` carry nothing: zero in x, zero weight rows and columns and biases in every convolution."""
    for q in chans:
        x[..., q] = 0.0
        for lay in layers:
            for w, b in ((lay[0], lay[1]), (lay[2], lay[3])):
                w[q] = 0.0
                w[:, q] = 0.0
                b[q] = 0.0


def chain_channels(c, C, n):
    """n + 1 distinct channels ending in c: the route of a planted value through n convolutions."""
    ch = [(c + 5 * (n - i)) % C for i in range(n)] + [c]
    assert len(set(ch)) == n + 1
    return ch


def plant(x, layers, site, rows, c, x0, gain, b, tap=1):
    """-> (x, layers) with site (a key of STAGE) of channel c holding gain * x0 + b at positions `rows` of x (T, C) (an index or a slice)
    and b everywhere else -- through a route of otherwise silent channels: x[rows, ch0] = x0, unit centre taps up to the site's
    convolution, there the one weight `gain` (on tap `tap`: 1 = the same position).  No other channel sees any of it: the value
    reaches this site alone (and whatever a later stage makes of channel c, which has no other input: the residual path of a Y)."""
    x, layers = _clone(x, layers)
    n = STAGE[site]
    ch = chain_channels(c, x.shape[-1], n + 1)
    _quiet(x, layers, ch)
    convs = [cv for lay in layers for cv in ((lay[0], lay[1]), (lay[2], lay[3]))]
    x[rows, ch[0]] = x0
    for i in range(n + 1):
        w, bias = convs[i]
        w[ch[i + 1], ch[i], tap if i == n else 1] = gain if i == n else 1.0
        if i == n:
            bias[ch[i + 1]] = b
    return x, tuple(tuple(lay) for lay in layers)


def plant_value(x, layers, site, t, c, v, k=1.0):
    return plant(x, layers, site, t, c, *decompose(v, k))


def plant_x(x, layers, t, c, v):
    """The raw trunk value v at (t, c) of a silent channel: site X alone (the fp32 y carries it on, unconverted)."""
    x, layers = _clone(x, layers)
    _quiet(x, layers, [c])
    x[t, c] = v
    return x, tuple(tuple(lay) for lay in layers)


def masked_bias(x, layers, site, c, Tb):
    """A bias of 2^17 on channel c of the site's convolution, cancelled at every position of the clip [0, Tb) by a product of -2^17:
    the site holds 0 inside the clip and 2^17 at every position of the tile grid outside it -- which the kernel masks (h IS zero
    there) or drops (y), and must not record."""
    return plant(x, layers, site, slice(0, Tb), c, 4096.0, -32.0, 2.0 ** 17)


def tap_gain(x, layers, gain=4.0):
    """The first conv1's weights times `gain` (an exact power of two), x divided by it: inside a clip h is what it was (the data stays
    exact), and every tap turns +-60000 past a clip's end into |h| >= 2^17."""
    return x / gain, ((layers[0][0] * gain,) + tuple(layers[0][1:]),) + tuple(layers[1:])


# ---------------------------------------------------------------------------------------------------------------------------------
# the planted cases of one launch kind of one form (fm: anything with p, C, x16, asrc, family, raw, act, lens_ok -- the Form of
# tests/test_gpu_resstack_launches.py), shared by the CPU emulation and the GPU launches
# ---------------------------------------------------------------------------------------------------------------------------------
EXACT_SLOPES = (0.5, 0.25)


def launch_kinds(fm, geo):
    """The launches of a form the cases run on: its pairs, its first single dilation on 1-D tiles and its first on folded tiles
    (geo(fm, T, dils): the plan's geometry)."""
    out = [d for d, _ in fm.launches() if len(d) == 2]
    singles = [d for d, _ in fm.launches() if len(d) == 1]
    for fold in (0, 1):
        out += [d for d in singles if geo(fm, 4096, d)["fold"] == fold][:1]
    return out


def exact_data(C, dils, T):
    seed = 1000 * C + 10 * sum(dils) + len(dils)
    row = R.EXACT_ROW_SINGLE if len(dils) == 1 else R.EXACT_ROW_PAIR
    return R.exact_trunk(1, T, C, seed)[0], tuple(R.exact_layer(C, seed + 1 + k, row) for k in range(len(dils)))


def positions(geo, T, dils):
    """First and last position, both sides of every tile seam of the plan's geometry `geo` at T, and (folded tiles: rows of d positions,
    TH rows per tile) both sides of the column seam and a position of the second tile column."""
    two = geo["TWo"]
    if geo["fold"]:
        seam = geo["TH"] * dils[0]
        pos = {0, T - 1, seam - 1, seam, two - 1, two, two + 1}
    else:
        pos = {0, T - 1} | {k * two - e for k in range(1, T // two + 1) for e in (0, 1)}
    return sorted(t for t in pos if 0 <= t < T)


def site_table(fm, pair):
    """[(site, the key of STAGE its value is planted at, (want_raw, want_act))]: the output set that isolates the site where the plan has
    one -- y alone for Y, ya alone for YA on the fp16 trunk (the fp32 y beside it converts nothing)."""
    inner = (fm.raw, fm.act)
    ystage = "Y2" if pair else "Y1"
    out = []
    if fm.p == 2 and not fm.x16 and not fm.asrc:
        out.append(("X", None, inner))
    out.append(("H", "H", inner))
    if pair:
        out += [("MID", "MID", inner), ("H2", "H2", inner)]
    if fm.p != 2:
        out.append(("Y", ystage, inner))          # (fp32 y of the split-bf16 forms: nothing is converted anywhere)
    else:
        if fm.x16 and not fm.asrc:
            out.append(("Y", ystage, (True, False)))
        out.append(("YA", ystage, (not fm.x16, True)))
    return out


def _case(kind, site, x, layers, sets, slopes=EXACT_SLOPES, lens=None, **kw):
    return dict(kind=kind, site=site, x=x if x.dim() == 3 else x[None], layers=layers, want_raw=sets[0], want_act=sets[1], slope=slopes[0],
                act_slope=slopes[1], exact=slopes == EXACT_SLOPES, lens=lens, **kw)


def site_cases(fm, dils, T, pos):
    """3a: every site of the form alone (where the arithmetic allows), the value at `pos` x channels {0, C/2 - 1, C/2, C - 1} zipped
    (every placement one must-raise and one must-not-raise value, the first placement all six), then: exactly 65504 (no verdict),
    +inf / NaN at the fp32 site X, and -2^17 in front of a LeakyReLU that runs before the conversion at slopes 0.01 and 0.2."""
    C, pair = fm.C, len(dils) == 2
    x, layers = exact_data(C, dils, T)
    chans = (0, C // 2 - 1, C // 2, C - 1)
    pl = [(t, chans[i % 4]) for i, t in enumerate(pos)]
    pl += [(pos[0], chans[i]) for i in range(len(pl), 4)]
    for site, stage, sets in site_table(fm, pair):
        # a site behind a LeakyReLU receives a negative v as slope * (v / slope): the exact slopes are powers of two
        behind = site in ("X", "MID", "YA") or (site in ("H", "H2") and PACKED[fm.family] == "after")
        inv = 1.0 / EXACT_SLOPES[1 if site == "YA" else 0]

        def mk(t, c, v, through=True):
            k = inv if (behind and through and v < 0) else 1.0
            return plant_x(x, layers, t, c, k * v) if stage is None else plant_value(x, layers, stage, t, c, v, k)
        for i, (t, c) in enumerate(pl):
            vals = RAISE_VALUES + QUIET_VALUES if i == 0 else (RAISE_VALUES[i % 4], QUIET_VALUES[i % 2])
            for v in vals:
                yield _case("site", site, *mk(t, c, v), sets, t=t, c=c, v=v)
        t, c = pl[1]
        yield _case("65504", site, *mk(t, c, 65504.0), sets, t=t, c=c, v=65504.0)
        if fm.p != 2:
            continue
        if site == "X":
            for v in (float("inf"), float("nan")):
                yield _case("nonfinite", site, *mk(t, c, v), sets, t=t, c=c, v=v)
        if site in ("X", "YA") or (site in ("H", "H2") and PACKED[fm.family] == "after"):
            for slopes in ((0.01, 0.2), (0.2, 0.01)):   # slope * v is what is converted
                yield _case("negative", site, *mk(t, c, -2.0 ** 17, False), sets, slopes, t=t, c=c, v=-2.0 ** 17)
                yield _case("negative", site, *mk(t, c, 2.0 ** 17), sets, slopes, t=t, c=c, v=2.0 ** 17)


PAST_F16 = (60000.0, -60000.0)
PAST_F32 = (float("inf"), float("nan"), 1e30, -1e30)


def outside_cases(fm, dils, T3, lens_sets, geo):
    """3b: nothing outside the clip raises the flag.  Batches of three with per-clip lengths, x past each clip's end +-60000 (fp16 trunk)
    or +inf / NaN / +-1e30 (fp32 trunk) under conv1 weights of gain 4; sequences of one and of seam + 1 positions with a bias of 2^17
    at each site, cancelled inside the sequence (must not raise) and not (must raise); and (1-D tiles) a value of 40000 next to a tile
    seam under two unit taps of conv2: both outputs it reaches hold 40000, the tile's edge pixel -- computed from clamped rows,
    never stored -- 80000."""
    C, pair = fm.C, len(dils) == 2
    x, layers = exact_data(C, dils, T3)
    xg, gained = tap_gain(x, layers)
    if fm.lens_ok:
        for sets in dict.fromkeys(s for _, _, s in site_table(fm, pair)):
            for lens in lens_sets:
                xb = torch.empty(3, T3, C)
                fill = PAST_F16 if fm.x16 else PAST_F32
                for b, Tb in enumerate(lens):
                    xb[b] = torch.tensor([fill[(b + ch) % len(fill)] for ch in range(C)])[None, :]
                    xb[b, :Tb] = xg[:Tb]
                yield _case("past_end", None, xb, gained, sets, lens=list(lens), v=0.0)
    seam = geo["TH"] * dils[0] if geo["fold"] else geo["TWo"]
    c = C // 2
    for T in (1, seam + 1):
        for site, stage, sets in site_table(fm, pair):
            if stage is None:
                continue
            yield _case("masked_bias", site, *masked_bias(x[:T], layers, stage, c, T), sets, t=T, c=c, v=0.0)
            yield _case("bias", site, *plant(x[:T], layers, stage, slice(0, 0), c, 0.0, 32.0, 2.0 ** 17), sets, t=T, c=c, v=2.0 ** 17)
    if not geo["fold"] and fm.p == 2:
        two, sets = geo["TWo"], site_table(fm, pair)[-1][2]
        for t, taps in ((two - 1, (0, 1)), (two, (1, 2))):   # the left edge pixel of the second tile, the right one of the first
            stage = "Y2" if pair else "Y1"
            n = STAGE[stage]
            xe, le = plant(x, layers, stage, t, c, 1250.0, 1.0, 0.0, tap=taps[0])
            le = [list(lay) for lay in le]
            ch = chain_channels(c, C, n + 1)
            le[n // 2][2][c, ch[n], taps[1]] = 1.0          # the second unit tap of the last conv2
            le[n // 2][0][ch[n], ch[n - 1], 1] = 32.0       # its conv1 delivers h = 32 * 1250 = 40000
            yield _case("edge_pixel", "Y", xe, tuple(tuple(lay) for lay in le), sets, t=t, c=c, v=40000.0)
