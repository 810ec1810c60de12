"""VFX_FLAG_F16_SATURATED, the one device-side guard of the 16-bit vocoder, one launch at a time: every case clears the handle's flag
word, launches once through the plan's own entry points (vfx_op_voc_resblock / _upsample / _conv1d / _final), reads the word, and
asserts that the bit equals the verdict of tests/f16_flag_ref.py's oracle (never undecided: asserted of the constructed data), that no
other bit is set, and that the stored outputs are the float64 values of the CLAMPED arithmetic bit for bit where the data is exact --
a saturated value is stored as +-65504, not as an infinity, not wrapped.

  a. every conversion site of every fused ResStack form fires alone: one planted value (tests/f16_flag_ref.py: plant) at the first and
     last position, both sides of every tile seam the plan reports, the second tile column of a folded tile; channels 0, C/2 - 1,
     C/2, C - 1 (every wave column, both lane halves, never only lane 0).  Where a form cannot isolate a site -- an fp32 trunk value
     also enters y through the residual, a pair's y1 is its second layer's residual -- the oracle says which other sites fire.
  b. nothing outside the clip raises it: +-60000 / inf / NaN / 1e30 past each clip's end under conv1 gains of 4, a bias of 2^17 that only
     masked positions keep, the never-stored edge pixels of a tile.
  c. the upsamplers on k_up16 and on the phased k_conv, every output phase, the same flag word from both kernels.
  d. the conv1d builder: the condnet's ELU prologue and activated output, the k7 reflection.
  e. what never raises it: the tail, and every planted ResStack case on the split-bf16 forms (no fp16 anywhere).
Split-bf16 forms run the same planted data: nothing is converted, so the bit stays down and y holds 2^17 itself."""
import pytest
import torch
import torch.nn.functional as F

import f16_flag_ref as Fr
import resstack_f64 as R
from test_gpu_resstack_launches import FORMS, SKIP, _bits, _family, _geo, _handle, _shapes, _tuned

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# fused ResStack launches
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = [(f, d) for f in FORMS for d in Fr.launch_kinds(f, _geo)]
FIXTURE_CASES = [c for c in CASES if c[0].tuning == 0]
TUNED_CASES = [c for c in CASES if c[0].tuning != 0]


def _ids(cases):
    return ["%s-d%s" % (f.name, "_".join(str(d) for d in dils)) for f, dils in cases]


def _launch(eng, form, dils, case, x=None, lens=None):
    """-> (flag word of this launch alone, y, ya)."""
    layers = case["layers"]
    eng.take_flags()
    y, ya, info = eng.op_voc_resblock(case["x"] if x is None else x, layers[0], dils[0], layer2=layers[1] if len(dils) == 2 else None,
                                      dil2=dils[1] if len(dils) == 2 else 0, slope=case["slope"], act_slope=case["act_slope"],
                                      want_raw=case["want_raw"], want_act=case["want_act"], lens=lens)
    flags = eng.take_flags()
    _family(form, info, (form.name, dils, case["kind"]))
    return flags, y, ya


def _oracle(eng, form, dils, case):
    """-> (verdict, per-clip references, whether the data is exact): the oracle over every clip of the launch."""
    B, T, _ = case["x"].shape
    raised, undecided, refs, exact = False, False, [], case["exact"]
    for b in range(B):
        Tb = T if case["lens"] is None else case["lens"][b]
        kw = dict(x16=form.x16, asrc=form.asrc, sat=Fr.PACKED[form.family] if form.p == 2 else None)
        args = (case["x"][b, :Tb], case["layers"], dils, case["slope"], case["act_slope"], form.p, eng.tol['conv'])
        ref = R.resstack_ref(*args, bounds=not exact, **kw)
        stored = dict(y16=form.x16 and not form.asrc and case["want_raw"], ya=case["want_act"])
        if exact and form.p == 2 and case["kind"] != "nonfinite" and not Fr.exact_sat_fits(ref, **stored):
            # (slope * v of a negative v in front of a LeakyReLU is no fp16 number: this case is held to the bars instead)
            assert case["v"] < 0, (form.name, dils, case["kind"], case["site"], case["v"], "the planted data is not exact")
            exact = False
            ref = R.resstack_ref(*args, bounds=True, **kw)
        sites = Fr.resstack_sites(ref, p=form.p, x16=form.x16, asrc=form.asrc, family=form.family, pair=len(dils) == 2,
                                  want_raw=case["want_raw"], want_act=case["want_act"], act_slope=case["act_slope"], exact=exact)
        v, per = Fr.verdict(sites) if sites else (False, {})
        raised, undecided = raised or v is True, undecided or v is None
        ref["per"] = per
        refs.append(ref)
    return (True if raised else None if undecided else False), refs, exact


def _check(eng, form, dils, case, say):
    what = (form.name, dils, case["kind"], case["site"], case.get("t"), case.get("c"), case.get("v"), case["slope"], case["act_slope"],
            case["want_raw"], case["want_act"], case["lens"])
    want, refs, exact = _oracle(eng, form, dils, case)
    flags, y, ya = _launch(eng, form, dils, case, lens=case["lens"])
    say.append("%s -> flags %d, oracle %s %s" % (what, flags, want, refs[0]["per"]))
    if case["kind"] == "65504":     # the one value on which the record types differ: no verdict
        assert want is not True and (flags & ~Fr.FLAG) == 0, what
    else:
        assert want is not None, (what, "the oracle is undecided", refs[0]["per"])
        assert flags == (Fr.FLAG if want else 0), (what, "flag word %d, the oracle says %s" % (flags, want), [r["per"] for r in refs])
    if case["kind"] == "site" and form.p == 2 and case["v"] > 0:   # the site the value was planted at is the one the verdict rests on
        assert refs[0]["per"][case["site"]] is (case["v"] >= Fr.RAISE), (what, refs[0]["per"])
    y16 = form.x16 and not form.asrc
    for b, ref in enumerate(refs):
        Tb = ref["y"].shape[0]
        for got, key, bar in ((y, "y16" if (y16 and form.p == 2) else "y", "bar_y16" if y16 else "bar_y32"), (ya, "ya", "bar_ya")):
            if got is None:
                continue
            assert torch.isnan(got[b, Tb:]).all(), (what, b, key, "written past the clip's end")
            g = got[b, :Tb].cpu().double()
            if case["kind"] == "nonfinite":
                continue
            if exact:
                assert torch.equal(g, ref[key]), (what, b, key, (g != ref[key]).nonzero()[:4].tolist())
            elif want is False:
                assert ((g - ref[key]).abs() <= ref[bar]).all(), (what, b, key, ((g - ref[key]).abs() / ref[bar]).max().item())
            else:
                assert torch.isfinite(g).all(), (what, b, key, "a saturated value was not stored as a finite number")
    if case["kind"] == "past_end":      # every clip equals its batch-of-one launch bit for bit, which raises nothing either
        for b, Tb in enumerate(case["lens"]):
            f1, y1, ya1 = _launch(eng, form, dils, case, x=case["x"][b:b + 1, :Tb])
            assert f1 == 0, (what, b, "the clip's batch-of-one launch raised %d" % f1)
            for got, solo in ((y, y1), (ya, ya1)):
                if got is not None:
                    assert torch.equal(_bits(got[b, :Tb]), _bits(solo[0])), (what, b, "differs from the clip's batch-of-one launch")


def _run(eng, form, dils, part):
    Ts, T3, lens_sets = _shapes(form, dils)
    geo = _geo(form, T3, dils)
    cases = Fr.site_cases(form, dils, T3, Fr.positions(geo, T3, dils)) if part == "site" else Fr.outside_cases(form, dils, T3, lens_sets, geo)
    say = []
    try:
        for case in cases:
            _check(eng, form, dils, case, say)
    finally:
        print("\n".join(say))


@pytest.mark.parametrize("form,dils", FIXTURE_CASES, ids=_ids(FIXTURE_CASES))
def test_each_site_fires_alone(engine, form, dils):
    """(a), and (e) on the split-bf16 forms: the same planted values convert nothing there."""
    eng = _handle(form, engine)
    if eng is None:
        pytest.skip(SKIP)
    _run(eng, form, dils, "site")


@pytest.mark.parametrize("form,dils", TUNED_CASES, ids=_ids(TUNED_CASES))
def test_each_site_fires_alone_tuning_variants(form, dils):
    """... k_resblock's 16-bit form (H behind the fp32 LeakyReLU), the fp32 trunks (site X) and the layers of dilation 1 and 3 alone."""
    _run(_tuned(form.tuning), form, dils, "site")


@pytest.mark.parametrize("form,dils", FIXTURE_CASES, ids=_ids(FIXTURE_CASES))
def test_nothing_outside_the_clip_raises_it(engine, form, dils):
    """(b)."""
    eng = _handle(form, engine)
    if eng is None:
        pytest.skip(SKIP)
    _run(eng, form, dils, "outside")


@pytest.mark.parametrize("form,dils", TUNED_CASES, ids=_ids(TUNED_CASES))
def test_nothing_outside_the_clip_raises_it_tuning_variants(form, dils):
    _run(_tuned(form.tuning), form, dils, "outside")


# ---------------------------------------------------------------------------------------------------------------------------------
# upsamplers: ConvTranspose1d(k = 2 s, stride s) on the activated fp16 source, exact data (integers, weights in {-1, 0, 1}, LeakyReLU
# slope 0.5 on the host), one planted product 32 * x0 + b on an otherwise silent (input channel, output channel) pair
# ---------------------------------------------------------------------------------------------------------------------------------
UP_SLOPE_EXACT = 0.5
_UP_ENGINES = {}


def _up_engine(tuning):
    if tuning not in _UP_ENGINES:
        from voicefixer_main_amd.engine import Engine
        _UP_ENGINES[tuning] = Engine("cuda:0", config={"precision": 2, "tuning": tuning})
    return _UP_ENGINES[tuning]


def _up_data(Cin, s, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    Cout = Cin // 2
    x = torch.randint(-4, 5, (B, T, Cin), generator=g).float()
    w = torch.zeros(Cin, Cout * 2 * s)
    for i in range(Cin):   # four taps per input channel
        idx = torch.randperm(Cout * 2 * s, generator=g)[:4]
        w[i, idx] = (torch.randint(0, 2, (4,), generator=g) * 2 - 1).float()
    b = torch.randint(-2, 3, (Cout,), generator=g).float() * 0.5
    return x, w.reshape(Cin, Cout, 2 * s), b


def _up_plant(x, w, b, bi, t, k, ci, co, v):
    x, w, b = x.clone(), w.clone(), b.clone()
    x0, gain, bias = Fr.decompose(v)
    x[..., ci] = 0.0
    w[ci] = 0.0
    w[:, co] = 0.0
    x[bi, t, ci], w[ci, co, k], b[co] = x0, gain, bias
    return x, w, b


def _up_ref(x, w, b, s):
    """x (T, Cin) of ONE clip -> float64 (T s, Cout): the transposed convolution on the fp16 operands, unclamped."""
    pad, opad = s // 2 + s % 2, s % 2
    a = F.leaky_relu(x, UP_SLOPE_EXACT).clamp(-65504.0, 65504.0).half().double().T[None]
    return F.conv_transpose1d(a, w.double(), b.double(), stride=s, padding=pad, output_padding=opad)[0].T


def _up_check(eng, Cin, s, x, w, b, lens, act_slope, want, what, up16):
    eng.take_flags()
    _, ya, used = eng.op_voc_upsample(x, w.numpy(), b.numpy(), s, UP_SLOPE_EXACT, src_act=True, want_raw=False, act_slope=act_slope, lens=lens)
    flags = eng.take_flags()
    assert used == up16, (what, "ran on k_up16: %s" % used)
    raised = False
    for bi in range(x.shape[0]):
        Tb = x.shape[1] if lens is None else lens[bi]
        ref = _up_ref(x[bi, :Tb], w, b, s)
        out = F.leaky_relu(ref, act_slope)
        v = Fr.site_verdict(out, torch.zeros_like(out))   # exact data: every sum is a small multiple of 1/2, or the planted product
        assert v is not None, (what, "the oracle is undecided")
        raised = raised or v
        assert torch.equal((ref * 4).round(), ref * 4) and ref.abs().max() <= 2.0 ** 17, (what, "the data is not exact")
        assert torch.equal(ya[bi, :Tb * s].cpu().double(), out.clamp(-65504.0, 65504.0)), (what, bi, "stored output")
        assert torch.isnan(ya[bi, Tb * s:]).all(), (what, bi, "written past the clip's end")
    if want is not None:
        assert raised == want, (what, "the oracle says %s of data built for %s" % (raised, want))
    assert flags == (Fr.FLAG if raised else 0), (what, "flag word %d, the oracle says %s" % (flags, raised))
    return flags


def _up_cases(Cin, s, T, up16):
    """(x, w, b, lens, must raise, what): every output phase r < s (tap k = pad + r of the planted input position), the first and the
    last output; per-clip lengths with +-60000 past each clip's end; and a product of 2^17 that only an output past the clip's end
    receives (tap s + pad of the clip's last position: output Tb s, dropped)."""
    pad = s // 2 + s % 2
    Cout = Cin // 2
    x, w, b = _up_data(Cin, s, 1, T, 100 * Cin + 10 * s + T)
    chans = [(0, 0), (Cin // 2 - 1, Cout // 2 - 1), (Cin // 2, Cout // 2), (Cin - 1, Cout - 1)]
    for r in range(s):
        t = (0, T - 1, T // 2)[r % 3] if r not in (0, s - 1) else (0 if r == 0 else T - 1)
        ci, co = chans[r % 4]
        vr, vq = Fr.RAISE_VALUES[r % 4], Fr.QUIET_VALUES[r % 2]
        if not up16 and vr == -65520.0:
            vr = -2.0 ** 17   # (0.25 * -65520 is no fp16 number: the stored output would not be exact)
        yield _up_plant(x, w, b, 0, t, pad + r, ci, co, vr) + (None, True, ("phase", r, t, ci, co, vr))
        yield _up_plant(x, w, b, 0, t, pad + r, ci, co, vq) + (None, False, ("phase", r, t, ci, co, vq))
    if T >= 3:
        lens = [T, max(1, T - 1 - T // 3), 1]
        xb = torch.empty(3, T, Cin)
        for bi, Tb in enumerate(lens):
            xb[bi] = torch.tensor([Fr.PAST_F16[(bi + c) % 2] for c in range(Cin)])[None, :]
            xb[bi, :Tb] = x[0, :Tb]
        yield xb, w, b, lens, False, ("past_end", lens)
        xs, ws, bs = _up_plant(xb, w, b, 1, lens[1] - 1, s + pad, Cin // 2, Cout // 2, 2.0 ** 17)
        xs[1, lens[1]:, Cin // 2] = 60000.0
        yield xs, ws, bs, lens, False, ("dropped_output", lens)
    if T % 128 not in (0,):   # the sequence ends inside a tile: the same product past the last output of a tensor without lengths
        yield _up_plant(x, w, b, 0, T - 1, s + pad, Cin // 2, Cout // 2, 2.0 ** 17) + (None, False, ("dropped_output", T))


@pytest.mark.parametrize("Cin,s", [(128, 2), (128, 3), (128, 7), (128, 9), (256, 3), (256, 7), (512, 3), (512, 7), (64, 3), (64, 7)])
def test_upsampler_flag(Cin, s):
    """(c): Cin = 128 / 256 run on k_up16 (asserted), 512 / 64 on the phased k_conv; the fp16 trunk output (act_slope 1) of the former,
    the activated output (slope 0.25: a negative -2^17 becomes -32768 and is quiet) of the latter.  The k_up16 launches are repeated
    on a VFX_TUNE_NO_FUSED_UPSAMPLERS handle: the same flag word from both kernels."""
    from voicefixer_main_amd import _lib
    up16 = Cin in (128, 256)
    eng = _up_engine(0)
    for T in ((1, 127, 129) if Cin <= 256 else (1, 129)):
        for x, w, b, lens, want, what in _up_cases(Cin, s, T, up16):
            what = (Cin, s, T) + what
            if not up16 and what[3] == "phase" and what[-1] < 0:
                want = None   # (through the activation: the oracle decides)
            flags = _up_check(eng, Cin, s, x, w, b, lens, 1.0 if up16 else 0.25, want, what, up16)
            if up16:
                other = _up_check(_up_engine(_lib.TUNE_NO_FUSED_UPSAMPLERS), Cin, s, x, w, b, lens, 1.0, want, what + ("phased",), False)
                assert flags == other, (what, "k_up16 %d, the phased k_conv %d" % (flags, other))


# ---------------------------------------------------------------------------------------------------------------------------------
# the conv1d builder (k_conv in the 16-bit mode): SRC = the launch's own prologue on a raw fp32 source (src_act = 0; a source the
# producer activated arrives as fp16 and is converted by nobody), OUT = the activated fp16 output of conv_epilogue.h
# ---------------------------------------------------------------------------------------------------------------------------------
def _conv_data(Cin, Cout, K, B, T, seed, lo=-4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(lo, 5, (B, T, Cin), generator=g).float()
    w = torch.zeros(Cout, Cin * K)
    for o in range(Cout):
        idx = torch.randperm(Cin * K, generator=g)[:6]
        w[o, idx] = (torch.randint(0, 2, (6,), generator=g) * 2 - 1).float()
    return x, w.reshape(Cout, Cin, K), torch.randint(-2, 3, (Cout,), generator=g).float() * 0.5


def _conv_run(engine, x, w, b, *, dil=1, reflect=False, src_act, act, slope, next_act, next_slope=1.0, want_raw, residual=None,
              res_value=None, lens=None, exact=True, what=()):
    """One launch; SRC and OUT from the float64 convolution of the fp16 operands (exact data: bar zero; exact = False: the bar of a
    dozen fp32 roundings, 2^-20 relative).  res_value (T, Cout) float64: what the epilogue adds (the inverted activated trunk)."""
    from launch_parity_f64 import _act32, _act64
    mode16 = engine.tol['name'] == 'fp16-vocoder'
    K = w.shape[2]
    engine.take_flags()
    y, ya = engine.op_voc_conv1d(x, w.numpy(), b.numpy(), dil=dil, reflect=reflect, src_act=src_act, act=act, slope=slope,
                                 residual=residual, residual_act=residual is not None, want_raw=want_raw, next_act=next_act,
                                 next_slope=next_slope, lens=lens)
    flags = engine.take_flags()
    if not mode16:   # (e): no fp16 anywhere
        assert flags == 0, (what, flags)
        return
    sites, raised = {}, False
    for bi in range(x.shape[0]):
        Tb = x.shape[1] if lens is None else lens[bi]
        pre = _act32(x[bi, :Tb], act, slope)
        a = torch.nan_to_num(pre, nan=-65504.0).clamp(-65504.0, 65504.0).half().double().T[None]
        if reflect:
            ref = F.conv1d(F.pad(a, (K // 2, K // 2), mode="reflect"), w.double(), b.double())[0].T
        else:
            ref = F.conv1d(a, w.double(), b.double(), padding=dil * (K // 2), dilation=dil)[0].T
        if res_value is not None:
            ref = ref + res_value[bi, :Tb]
        if not src_act:
            sites["SRC"] = (pre.double(), torch.zeros_like(pre, dtype=torch.float64))
        if next_act:
            out = _act64(ref, next_act, next_slope)
            sites["OUT"] = (out, torch.zeros_like(out) if exact else 2.0 ** -20 * out.abs())
        v, per = Fr.verdict(sites) if sites else (False, {})
        assert v is not None, (what, "the oracle is undecided", per)
        raised = raised or v
        if exact and torch.isfinite(pre).all():
            if y is not None:
                assert torch.equal(y[bi, :Tb].cpu().double(), ref), (what, bi, "y")
            if ya is not None and next_act == 1:
                assert torch.equal(ya[bi, :Tb].cpu().double(), out.clamp(-65504.0, 65504.0)), (what, bi, "ya")
            if ya is not None and next_act == 2:   # ELU of a negative value lies in (-1, 0): within an fp16 ulp there (2^-11)
                assert ((ya[bi, :Tb].cpu().double() - out.clamp(max=65504.0)).abs() <= torch.where(ref < 0, 2.0 ** -11, 0.0)).all(), (what, bi, "ya")
        for t in (y, ya):
            if t is not None:
                assert torch.isnan(t[bi, Tb:]).all(), (what, bi, "written past the clip's end")
    assert flags == (Fr.FLAG if raised else 0), (what, "flag word %d, the oracle says %s" % (flags, raised), per)


def _conv_plant(x, w, b, t, k, ci, co, v):
    """x[0, t, ci] * w[co, ci, k] + b[co] = v on a silent (input channel, output channel) pair."""
    x, w, b = x.clone(), w.clone(), b.clone()
    x0, gain, bias = Fr.decompose(v)
    x[..., ci] = 0.0
    w[:, ci] = 0.0
    w[co] = 0.0
    x[0, t, ci], w[co, ci, k], b[co] = x0, gain, bias
    return x, w, b


def _conv_src_plant(x, w, t, ci, v):
    x, w = x.clone(), w.clone()
    x[..., ci] = 0.0
    w[:, ci] = 0.0
    x[0, t, ci] = v
    return x, w


def test_condnet_layers_flag(engine):
    """(d): the first condnet layer converts the raw conditioning in its prologue (SRC, no activation: both signs raise); both layers
    store ELU(conv) (OUT): a large negative value becomes about -1 and is quiet, the same value positive raises.  A source the
    producer already activated (layer i > 0) holds ELU(-2^17) = -1: nothing to convert, quiet."""
    for T, B in ((1, 1), (129, 3)):
        lens = None if B == 1 else [T, 86, 1]
        x, w, b = _conv_data(128, 512, 3, B, T, 40 + T)
        kw = dict(src_act=False, act=0, slope=1.0, next_act=2, want_raw=False, lens=lens)
        for i, v in enumerate(Fr.RAISE_VALUES + Fr.QUIET_VALUES):
            t, ci, co = (0, T - 1)[i % 2], (0, 63, 64, 127)[i % 4], (0, 255, 256, 511)[i % 4]
            xs, ws = _conv_src_plant(x, w, t, ci, v)
            _conv_run(engine, xs, ws, b, what=("condnet0", "SRC", T, t, ci, v), **kw)
            _conv_run(engine, *_conv_plant(x, w, b, t, 1, ci, co, v), what=("condnet0", "OUT", T, t, co, v), **kw)
        if lens is not None:   # large values past each clip's end: masked in the prologue, in front of the conversion
            xs = x.clone()
            for bi, Tb in enumerate(lens):
                xs[bi, Tb:] = 1e30 * (-1.0) ** bi
            _conv_run(engine, xs, w, b, what=("condnet0", "past_end", T), **kw)
        x, w, b = _conv_data(512, 512, 3, B, T, 50 + T, lo=0)   # (non-negative: the producer's ELU is the identity, exactly)
        kw = dict(src_act=True, act=2, slope=1.0, next_act=2, want_raw=False, lens=lens)
        for i, v in enumerate((2.0 ** 17, -2.0 ** 17, 65520.0, 65472.0)):
            t, ci, co = (0, T - 1)[i % 2], (0, 255, 256, 511)[i % 4], (511, 256, 255, 0)[i % 4]
            _conv_run(engine, *_conv_plant(x, w, b, t, 1, ci, co, v), what=("condnet", "OUT", T, t, co, v), **kw)
        xs, ws = _conv_src_plant(x, w, 0, 256, -2.0 ** 17)
        _conv_run(engine, xs, ws, b, what=("condnet", "activated source", T), **kw)


@pytest.mark.parametrize("T", [4, 9, 130])
def test_k7_reflect_conv_flag(engine, T):
    """(d): ReflectionPad1d(3) + k7, 512 -> 1024, LeakyReLU output (slope 0.25): the planted source position among the first and last
    four, which the reflection reads twice -- every output its tap reaches holds the value."""
    x, w, b = _conv_data(512, 1024, 7, 1, T, 60 + T, lo=0)
    kw = dict(reflect=True, src_act=True, act=2, slope=1.0, next_act=1, next_slope=0.25, want_raw=False)
    pos = sorted(set(range(min(4, T))) | set(range(max(0, T - 4), T)))
    vals = (2.0 ** 17, 65520.0, 65472.0, -2.0 ** 17, -65472.0)
    for i, t in enumerate(pos):
        ci, co, v = (0, 255, 256, 511)[i % 4], (0, 511, 512, 1023)[i % 4], vals[i % 5]
        _conv_run(engine, *_conv_plant(x, w, b, t, i % 7, ci, co, v), what=("k7", T, t, i % 7, co, v), **kw)


def test_raw_32_channel_layer_flag(engine):
    """(d): the 32-channel raw form converts LeakyReLU(x) in the launch's prologue (SRC) and stores fp32: +2^17, +-65520 (slope 0.5:
    -2^17 becomes -65536) and inf / NaN raise, +-65472 are quiet, and -2^17 is quiet at slopes 0.01 and 0.2."""
    for T, dil in ((20, 27), (131, 1)):
        x, w, b = _conv_data(32, 32, 3, 1, T, 70 + T)
        for i, v in enumerate((2.0 ** 17, -2.0 ** 17, 65520.0, 65472.0, -65472.0, float("inf"), float("nan"))):
            xs, ws = _conv_src_plant(x, w, (0, T - 1)[i % 2], (0, 15, 16, 31)[i % 4], v)
            _conv_run(engine, xs, ws, b, dil=dil, src_act=False, act=1, slope=0.5, next_act=0, want_raw=True, what=("raw32", T, dil, v))
        for slope in (0.01, 0.2):
            xs, ws = _conv_src_plant(x, w, T // 2, 16, -2.0 ** 17)
            _conv_run(engine, xs, ws, b, dil=dil, src_act=False, act=1, slope=slope, next_act=0, want_raw=True, exact=False,
                      what=("raw32", T, dil, "negative", slope))


def test_c512_layer_with_the_inverted_trunk_flag(engine):
    """(d): conv2 of a C = 512 layer in the 16-bit mode adds the trunk recovered from its activated fp16 form, min(v, v / 0.01): a large
    negative trunk value re-enters y near -65504 / 0.01 in fp32, and the output stores 0.01 y.  On its own that lands on the limit
    (undecided: not asserted); with a planted product of -2^17 beside it the output is about -66800 and must raise, with a trunk
    value of -60000 / 0.01 about -61300 and quiet."""
    if engine.tol['name'] != 'fp16-vocoder':
        pytest.skip("residual_act exists in the 16-bit mode only")
    import numpy as np
    T, C, slope = 130, 512, 0.01
    x, w, b = _conv_data(C, C, 3, 1, T, 90, lo=0)
    for t, co, r in ((0, 0, -6.5504e6), (T - 1, 511, -6.0e6), (64, 255, 3.0)):
        xs, ws, bs = _conv_plant(x, w, b, t, 1, 256, co, -2.0 ** 17)
        res = torch.zeros(1, T, C)
        res[0, t, co] = r
        v = F.leaky_relu(res, slope).clamp(-65504.0, 65504.0).half().float()
        inv = torch.minimum(v, v * (np.float32(1.0) / np.float32(slope))).double()
        _conv_run(engine, xs, ws, bs, src_act=True, act=1, slope=0.5, next_act=1, next_slope=slope, want_raw=False, residual=res,
                  res_value=inv, exact=False, what=("c512", t, co, r))


# ---------------------------------------------------------------------------------------------------------------------------------
# what must never raise it
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_f16", [False, True], ids=["f32-trunk", "f16-trunk"])
def test_the_tail_never_raises_it(engine, x_f16):
    """(e): vfx_op_voc_final converts nothing and tanh bounds its output -- an fp16 trunk full of +-65504, an fp32 trunk with 1e30."""
    B, T, C = 2, 300, 64
    x = torch.full((B, T, C), 65504.0 if x_f16 else 1e30)
    x[:, ::2, 1::2] *= -1.0
    w = torch.zeros(1, C, 7)
    w[0, :, 3] = 1.0 / C
    engine.take_flags()
    wav = engine.op_voc_final(x, w.numpy(), 0.05, 0.2, x_f16=x_f16, lens=[300, 13]).cpu()
    assert engine.take_flags() == 0
    assert torch.isfinite(wav[0]).all() and torch.isfinite(wav[1, :13]).all() and wav[:, :13].abs().max() <= 1.0


def test_other_modes_never_raise_it(engine):
    """(e): the planted upsampler cases on the fp32 and split-bf16 handles -- no fp16 anywhere, the raw output holds 2^17 itself."""
    if engine.tol['name'] == 'fp16-vocoder':
        pytest.skip("the 16-bit mode is what the other tests of this file run")
    for x, w, b, lens, _, what in _up_cases(128, 3, 129, True):
        engine.take_flags()
        y, _, used = engine.op_voc_upsample(x, w.numpy(), b.numpy(), 3, UP_SLOPE_EXACT, src_act=True, want_raw=True, lens=lens)
        assert engine.take_flags() == 0 and not used, what
        for bi in range(x.shape[0]):
            Tb = x.shape[1] if lens is None else lens[bi]
            # (the split-bf16 source is the hi + lo pair of the activated value: exact for these integers and halves)
            a = F.leaky_relu(x[bi, :Tb], UP_SLOPE_EXACT).double().T[None]
            ref = F.conv_transpose1d(a, w.double(), b.double(), stride=3, padding=2, output_padding=1)[0].T
            assert torch.equal(y[bi, :Tb * 3].cpu().double(), ref), (what, bi)
