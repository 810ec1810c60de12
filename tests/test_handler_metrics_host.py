"""CPU: the float64 references of the handler scores (tests/handler_metrics_f64.py) against the handlers' own formulas in torch
float64 (handlers.lsd / sispec / ssim), and the C surface of the scored restore entries."""
import os
import re

import numpy as np
import pytest
import torch

import handler_metrics_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(seed, T):
    rng = np.random.default_rng(seed)
    tgt = (10.0 ** rng.normal(-1.0, 1.0, size=(T, 128))).astype(np.float32)
    lg = (np.log10(tgt) + 0.3 * rng.normal(size=tgt.shape)).astype(np.float32)
    return lg, tgt


def _t(x):
    return torch.from_numpy(np.asarray(x, np.float64))[None, None]


@pytest.mark.parametrize("T,unify", [(7, False), (33, True), (75, False)])
def test_references_match_the_handlers_formulas(T, unify):
    from voicefixer_main_amd import handlers
    lg, tgt = _images(T, T)
    # from_log clips at 5.  The 1e5 pixels sit in the image's last corner: scipy's uniform_filter, which audio_metrics_f64.ssim is
    # built on, keeps a RUNNING sum along each axis, so every window behind a 1e10 term of x * x inherits its 1e-6 rounding residue
    # (4e-8 of the score with the pixels in the first corner); in the last corner no window lies behind them
    lg[-1, -5:] = 5.5
    lin = ref.from_log(lg)
    den = lin * 0.37 if unify else lin
    got = ref.gsr_scores(lg, lin, den, tgt)
    want = [float(handlers.lsd(_t(den), _t(tgt))), float(handlers.sispec(_t(lg), handlers.to_log(_t(tgt)))),
            float(handlers.sispec(_t(lin), _t(tgt))), float(handlers.ssim(_t(den), _t(tgt)))]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)
    est = np.abs(lin).astype(np.float32)
    got = ref.ssr_scores(est, tgt)
    want = [float(handlers.lsd(_t(est), _t(tgt))), float(handlers.sispec(handlers.to_log(_t(est)), handlers.to_log(_t(tgt)))),
            float(handlers.sispec(_t(est), _t(tgt))), float(handlers.ssim(_t(est), _t(tgt)))]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)


def test_from_log_is_the_models_from_log():
    from voicefixer_main_amd import models
    lg = np.linspace(-9.0, 7.0, 101)
    np.testing.assert_allclose(ref.from_log(lg), models.from_log(torch.from_numpy(lg)).numpy(), rtol=1e-14, atol=0)
    assert ref.KEYS == models.HANDLER_METRIC_KEYS


def test_an_all_zero_target_has_finite_scores():
    lg, tgt = _images(3, 9)
    s = ref.gsr_scores(lg, ref.from_log(lg), ref.from_log(lg), np.zeros_like(tgt))
    assert np.isfinite(s).all() and s[0] == pytest.approx(12.0, abs=1e-12) and s[2] == pytest.approx(-120.0, abs=1e-9)


def test_scored_entries_are_declared_and_bound():
    from voicefixer_main_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vfx.h")).read()
    thdr = open(os.path.join(ROOT, "include", "vfx_test.h")).read()
    assert re.search(r"#define VFX_N_HANDLER_METRICS 4\b", hdr) and _lib.N_HANDLER_METRICS == 4
    for name, nargs in (("vfx_restore_gsr_varlen_scored", 12), ("vfx_restore_ssr_varlen_scored", 10)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m and len(m.group(1).split(",")) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs
    for name, nargs in (("vfx_op_handler_metrics", 9), ("vfx_op_mel_metrics", 8)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, thdr)
        assert m and len(m.group(1).split(",")) == nargs and len(_lib.TEST_SIGNATURES[name][1]) == nargs
    # the unscored entries keep their signatures
    assert len(_lib.SIGNATURES["vfx_restore_gsr_varlen"][1]) == 9 and len(_lib.SIGNATURES["vfx_restore_ssr_varlen"][1]) == 7


def test_the_product_module_does_not_load_the_test_library():
    src = open(os.path.join(ROOT, "voicefixer_main_amd", "evaluation.py")).read()
    assert "load_test" not in src
