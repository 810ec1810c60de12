"""CPU checks of tests/f16_flag_ref.py, the oracle that tests/test_gpu_f16_flag_launches.py holds VFX_FLAG_F16_SATURATED to: on every
planted case of one 1-D and one folded geometry per kernel family, resstack_f64.emulate's saturation record (the kernels' rule: mask
the positions that do not count, then record !(|v| <= 65504)) gives the oracle's verdict, no case is undecided -- and each defect of
resstack_f64.FLAG_DEFECTS planted into the emulation flips the verdict of a case built for it, so the GPU tests can fail."""
import pytest
import torch

import f16_flag_ref as Fr
import resstack_f64 as R
from conftest import TOL
from test_gpu_resstack_launches import FORMS, _geo, _shapes

# one form per kernel family, and the fp32 trunk of resblock_r128 (site X; MID alone: its y stays fp32)
HOST_FORMS = [f for f in FORMS if f.name in ("rw-c64", "r128-c128", "w64-c256", "hionly-c64", "f32trunk-c128")]


def _kinds(form):
    """One launch on 1-D tiles (a pair where the form has pairs) and one on folded tiles."""
    kinds = Fr.launch_kinds(form, _geo)
    return [kinds[0], kinds[-1]]


def _cases(form, dils):
    Ts, T3, lens_sets = _shapes(form, dils)
    geo = _geo(form, T3, dils)
    yield from Fr.site_cases(form, dils, T3, Fr.positions(geo, T3, dils))
    yield from Fr.outside_cases(form, dils, T3, lens_sets, geo)


def _oracle(form, dils, case, b):
    Tb = case["x"].shape[1] if case["lens"] is None else case["lens"][b]
    kw = dict(x16=form.x16, asrc=form.asrc, sat=Fr.PACKED[form.family])
    args = (case["x"][b, :Tb], case["layers"], dils, case["slope"], case["act_slope"], 2, TOL[2]["conv"])
    exact = case["exact"]
    ref = R.resstack_ref(*args, bounds=not exact, **kw)
    stored = dict(y16=form.x16 and not form.asrc and case["want_raw"], ya=case["want_act"])
    if exact and case["kind"] != "nonfinite" and not Fr.exact_sat_fits(ref, **stored):
        assert case["v"] < 0, (form.name, dils, case["kind"], case["site"], case["v"], "the planted data is not exact")
        exact = False
        ref = R.resstack_ref(*args, bounds=True, **kw)
    sites = Fr.resstack_sites(ref, p=2, x16=form.x16, asrc=form.asrc, family=form.family, pair=len(dils) == 2, want_raw=case["want_raw"],
                              want_act=case["want_act"], act_slope=case["act_slope"], exact=exact)
    return Fr.verdict(sites)


def _emulated(form, dils, case, b, defect=None):
    Tb = case["x"].shape[1] if case["lens"] is None else case["lens"][b]
    rec = R.emulate(case["x"][b], Tb, case["layers"], dils, case["slope"], case["act_slope"], 2, x16=form.x16, asrc=form.asrc,
                    packed=Fr.PACKED[form.family] == "packed", defect=defect, record=True, want_raw=case["want_raw"],
                    want_act=case["want_act"])[2]
    return any(rec.values()), rec


def _verdicts(form, dils, case, defect=None):
    """-> (the oracle's verdict of the launch, the emulation's flag, the oracle's per-site verdicts of clip 0)."""
    want, got, per0 = False, False, None
    for b in range(case["x"].shape[0]):
        v, per = _oracle(form, dils, case, b)
        per0 = per if per0 is None else per0
        want = None if (v is None or want is None) else (want or v)
        got = got or _emulated(form, dils, case, b, defect)[0]
    return want, got, per0


LAUNCHES = [(f, d) for f in HOST_FORMS for d in _kinds(f)]
IDS = ["%s-d%s" % (f.name, "_".join(str(d) for d in dils)) for f, dils in LAUNCHES]


@pytest.mark.parametrize("form,dils", LAUNCHES, ids=IDS)
def test_healthy_emulation_gives_the_oracles_verdict(form, dils):
    n = 0
    for case in _cases(form, dils):
        want, got, per = _verdicts(form, dils, case)
        what = (form.name, dils, case["kind"], case["site"], case.get("t"), case.get("c"), case.get("v"), case["slope"], case["lens"])
        if case["kind"] == "65504":
            assert want is not True, what
            continue
        assert want is not None, (what, "undecided", per)
        assert got == want, (what, per)
        if case["kind"] in ("past_end", "masked_bias", "edge_pixel"):
            assert want is False, what
        if case["kind"] in ("bias", "nonfinite"):
            assert want is True, what
        n += 1
    assert n > 40


def _isolated(form, dils, site):
    """The first case of 3a in which the oracle lets site `site` alone raise the flag."""
    for case in _cases(form, dils):
        if case["kind"] == "site" and case["site"] == site:
            want, per = _oracle(form, dils, case, 0)
            if want is True and [k for k, v in per.items() if v] == [site]:
                return case
    return None


def test_a_silent_site_flips_its_isolated_case():
    """site_silent(s): every site has a form in which it fires alone, and there the emulation without that site's report stays quiet
    where the oracle says must raise."""
    flipped = set()
    for form, dils in LAUNCHES:
        for site in ("X", "H", "MID", "H2", "Y", "YA"):
            case = _isolated(form, dils, site)
            if case is None:
                continue
            assert _emulated(form, dils, case, 0)[0] is True
            got, rec = _emulated(form, dils, case, 0, "site_silent:" + site)
            assert got is False, (form.name, dils, site, rec)
            flipped.add((Fr.PACKED[form.family], site))
    for conv in ("packed", "after"):
        assert {(conv, s) for s in ("H", "YA")} <= flipped
    assert {s for _, s in flipped} == {"X", "H", "MID", "H2", "Y", "YA"}, flipped


@pytest.mark.parametrize("form,dils", [c for c in LAUNCHES if c[0].lens_ok], ids=[i for c, i in zip(LAUNCHES, IDS) if c[0].lens_ok])
def test_a_record_in_front_of_the_mask_flips_a_case_past_the_clips_end(form, dils):
    """record_before_mask (conv_common.h: the defect of round 4): what lies past a clip's end raises the flag."""
    n = 0
    for case in _cases(form, dils):
        if case["kind"] != "past_end":
            continue
        want, got, _ = _verdicts(form, dils, case, "record_before_mask")
        assert want is False and got is True, (form.name, dils, case["lens"])
        n += 1
    assert n >= 2


def test_a_predicate_that_ignores_nan_flips_the_nan_case():
    """record_ignores_nan: |x| > 65504 is false of a NaN; the kernels' !(|x| <= 65504) is not."""
    n = 0
    for form, dils in LAUNCHES:
        for case in _cases(form, dils):
            if case["kind"] == "nonfinite" and case["v"] != case["v"]:
                want, got, per = _verdicts(form, dils, case, "record_ignores_nan")
                assert want is True and got is False and _verdicts(form, dils, case)[1] is True, (form.name, dils, per)
                n += 1
    assert n >= 2


def test_thresholds_are_the_fp16_grid():
    """65520 is the midpoint of 65504 and 2^16 (everything from there up leaves the range under round-to-nearest), 65472 the largest
    fp16 below 65504; exactly 65504 is undecided."""
    assert float(torch.tensor(65504.0).half()) == 65504.0 and float(torch.tensor(65472.0).half()) == 65472.0
    assert float(torch.nextafter(torch.tensor(65504.0).half(), torch.tensor(0.0).half())) == Fr.QUIET
    assert Fr.RAISE == (65504.0 + 65536.0) / 2
    z = torch.zeros(1, dtype=torch.float64)
    assert Fr.site_verdict(z + 65520.0, z) is True and Fr.site_verdict(z - 65472.0, z) is False and Fr.site_verdict(z + 65504.0, z) is None
    assert Fr.site_verdict(z + 65520.0, z + 1.0) is None and Fr.site_verdict(z + float("nan"), z) is True
    for v in Fr.RAISE_VALUES + Fr.QUIET_VALUES + (65504.0,):
        x0, gain, b = Fr.decompose(v)
        assert gain * x0 + b == v and float(torch.tensor(x0).half()) == x0 and 2.0 ** -14 <= abs(gain) <= 1024.0
