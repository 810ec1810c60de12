"""GPU: the launches of the bi_gru / dnn analysis plans (csrc/analysis.hip: k_dense, k_gru_seq), one at a time through libvfx_test.so
(vfx_op_analysis_piece: the plan's own builder member over the handle's own packed weights), against the float64 forms and the
per-element bounds of tests/analysis_f64.py -- the fourth part of the launch-level series beside test_gpu_vocoder_launches.py,
test_gpu_resunet_launches.py and test_gpu_frontend_launches.py.  tests/test_analysis_f64_host.py shows on the CPU that the defects
these cases are there for (a wrong W_hh column in any of the three parts of the split, a stale input projection, b_hn or a bias or a
scalar BN folded in the wrong place, a backward pass started at T - 1, exchanged gates or halves) lie 100 times and more outside.

Every output starts as NaN and must come back finite inside the clips and exactly 0.0 past them; the input rows at and past lens[b]
are NaN (the xp rows of the GRU pieces and the mel of the residual included) and must not matter.  The GRU pieces are checked ONE
step at a time: y[t] against the float64 cell applied to the launch's own y[t -+ 1].

One engine in mode 1: the kernels are the same in every mode (test_gpu_analysis_modules.py holds the three modes to equal bytes); a
second one carries the recurrence-heavy weights (W_hh x 4, b_hn x 8)."""
import pytest
import torch

import analysis_f64 as R
from conftest import _make_engine
from test_analysis_modules_host import MAKERS
from test_gpu_frontend_launches import _margined

pytestmark = pytest.mark.gpu

# The smallest k of bar = D + k G (analysis_f64) that would have passed, i.e. what the device's log10f, expf, tanhf and division add
# beyond the derived part D, measured on an MI355X (ROCm 7) on 2026-10-20 over all the cases below: the largest value the tests print.
# All three came out 0: every error lay inside the derived part D alone (worst |err| / (D + 4 G): lin1 0.028, fc0 0.048, lin6 0.020,
# fc5 0.017, gru0 0.147, gru1 0.124), so k is the floor of 4.
IN_LOG_K_MEASURED = 0.0       # lin1, fc0: to_log in front of the sum
RESID_K_MEASURED = 0.0        # lin6, fc5: + to_log(mel)
GRU_K_MEASURED = 0.0          # gru0, gru1, both weight sets


def _k(measured):
    """max(4, the margined measurement capped at 16): floor and cap are conditions, not measurements -- a correct libm may be a couple
    of ulp off, and the defects lie far above the bar at k = 16."""
    return max(4.0, _margined(measured, R.K_CAP)) if measured > 0 else 4.0


K = {"lin1": _k(IN_LOG_K_MEASURED), "fc0": _k(IN_LOG_K_MEASURED), "lin6": _k(RESID_K_MEASURED), "fc5": _k(RESID_K_MEASURED),
     "gru0": _k(GRU_K_MEASURED), "gru1": _k(GRU_K_MEASURED)}
assert all(4.0 <= k <= 16.0 for k in K.values())


def _mid(module):
    from voicefixer_main_amd.engine import MODEL_DNN_MEL, MODEL_GRU_MEL
    return MODEL_GRU_MEL if module == "bi_gru" else MODEL_DNN_MEL


@pytest.fixture(scope="module")
def sds():
    gru = MAKERS["bi_gru"]()
    return {"bi_gru": gru, "dnn": MAKERS["dnn"](), "heavy": R.recurrence_heavy(gru)}


@pytest.fixture(scope="module")
def eng(sds):
    e = _make_engine(1)
    for module in ("bi_gru", "dnn"):
        e.load_state_dict(_mid(module), sds[module])
    return e


@pytest.fixture(scope="module")
def eng_heavy(sds):
    e = _make_engine(1)
    e.load_state_dict(_mid("bi_gru"), sds["heavy"])
    return e


def _run_case(e, sd, piece, B, T, lens, seed, scale=1.0):
    """One launch on NaN-padded inputs -> (|err| / D without G, smallest k, |err|), asserted against bar = D + K[piece] G."""
    xs = [R.nan_pad(x, lens) for x in R.piece_inputs(piece, B, T, seed, scale)]
    got = e.op_analysis_piece(_mid(R.module_of(piece)), piece, xs, lens=lens).cpu()
    ref, D, G = R.piece_ref(sd, piece, xs, lens, got=got)
    ratio, k, err = R.compare(got, ref, D, G, lens)
    worst = R.worst_over_bar(got, ref, D, G, K.get(piece, 0.0), lens)
    print("%s (%d, %d)%s scale %g: max |err| %.3g, |err| / bar %.3g, smallest k %.3g" %
          (piece, B, T, "" if lens is None else " lens", scale, err, worst, k))
    assert worst <= 1.0, (piece, (B, T), lens and lens[:4], "max |err| / bar = %.3g (smallest k %.3g, |err| %.3g)" % (worst, k, err))
    return worst, k


@pytest.mark.parametrize("piece", [p for m in ("bi_gru", "dnn") for p in R.PIECES[m] if p not in R.GRU_PIECES])
def test_dense_launch(eng, sds, piece):
    eng.take_flags()
    res = [_run_case(eng, sds[R.module_of(piece)], piece, B, T, lens, seed=100 + i)
           for i, (B, T, lens) in enumerate(R.DENSE_SHAPES + ([R.CHUNK_SHAPE] if piece in R.CHUNK_PIECES else []))]
    print("%s: worst |err| / bar %.3g, smallest k %.3g" % (piece, max(r[0] for r in res), max(r[1] for r in res)))
    assert eng.take_flags() == 0


@pytest.mark.parametrize("weights", ["synth", "heavy"])
@pytest.mark.parametrize("piece", R.GRU_PIECES)
def test_gru_launch(eng, eng_heavy, sds, piece, weights):
    e, sd = (eng_heavy, sds["heavy"]) if weights == "heavy" else (eng, sds["bi_gru"])
    e.take_flags()
    res = []
    for scale in (1.0, 4.0):
        for i, (B, T, lens) in enumerate(R.GRU_SHAPES + ([R.CHUNK_SHAPE] if piece in R.CHUNK_PIECES else [])):
            res.append(_run_case(e, sd, piece, B, T, lens, seed=100 + i, scale=scale))
    print("%s %s: worst |err| / bar %.3g, smallest k %.3g" % (piece, weights, max(r[0] for r in res), max(r[1] for r in res)))
    assert e.take_flags() == 0


@pytest.mark.parametrize("module", ["bi_gru", "dnn"])
def test_the_pieces_are_the_products_launches(eng, module):
    """Each piece's output fed to the next is Engine.analysis_mel, bit for bit."""
    B, T, lens = R.CHAIN_SHAPE
    mel = R.mel_input(B, T, seed=41)
    eng.take_flags()
    for frames in (None, lens):
        x = R.nan_pad(mel, frames).cuda()
        h = x
        for piece in R.PIECES[module]:
            h = eng.op_analysis_piece(_mid(module), piece, [h, x] if piece in R.MEL_RESID else [h], lens=frames)
        want = eng.analysis_mel(_mid(module), x, frames=frames)
        assert torch.equal(h, want), (module, frames, (h - want).abs().max().item())
    assert eng.take_flags() == 0


@pytest.mark.parametrize("module", ["bi_gru", "dnn"])
def test_negative_input_flag_comes_from_the_first_launch_alone(eng, module):
    """Today's behaviour: to_log in front of the first Linear (lin1 / fc0) raises FLAG_NEGATIVE_INPUT for a negative mel value in a live
    row; the residual's to_log (lin6 / fc5) reads the same tensor behind it in the plan and raises nothing itself.  A negative value in
    a row past lens[b] is never read and raises nothing."""
    from voicefixer_main_amd import _lib
    first, last = R.PIECES[module][0], R.PIECES[module][-1]
    B, T, lens = 2, 20, [20, 13]
    mel = R.mel_input(B, T, seed=3)
    live, dead = mel.clone(), mel.clone()
    live[1, 12, 127] = -1e-3
    dead[1, 13, 0] = -1e-3
    dead[1, 19, 127] = -1.0
    h = R.rand_input(B, T, 256, seed=4)
    eng.take_flags()
    eng.op_analysis_piece(_mid(module), first, [dead], lens=lens)
    eng.op_analysis_piece(_mid(module), last, [h, dead], lens=lens)
    assert eng.take_flags() == 0
    eng.op_analysis_piece(_mid(module), last, [h, live], lens=lens)
    eng.op_analysis_piece(_mid(module), last, [h, live])
    assert eng.take_flags() == 0
    eng.op_analysis_piece(_mid(module), first, [live], lens=lens)
    assert eng.take_flags() == _lib.FLAG_NEGATIVE_INPUT
    eng.op_analysis_piece(_mid(module), first, [dead])
    assert eng.take_flags() == _lib.FLAG_NEGATIVE_INPUT
