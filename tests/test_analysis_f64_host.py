"""CPU: the float64 launch references of tests/test_gpu_analysis_launches.py (tests/analysis_f64.py) chained together are the float64
restatement of the modules; a plain fp32 evaluation of every launch on the GPU test's inputs stays inside its bound at the cap k = 16;
and each of the defects the GPU test is there for lands at least 100 times outside that bound at an element that belongs to a clip."""
import numpy as np
import pytest
import torch

import analysis_f64 as R
from test_analysis_modules_host import MAKERS, reference_forward

F32 = torch.float32


@pytest.fixture(scope="module")
def sds():
    gru = MAKERS["bi_gru"]()
    return {"bi_gru": gru, "dnn": MAKERS["dnn"](), "heavy": R.recurrence_heavy(gru)}


def _sd_of(sds, piece, heavy=False):
    return sds["heavy"] if heavy else sds[R.module_of(piece)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the launches in fp32 (torch on the CPU), with the defects planted on request
# ---------------------------------------------------------------------------------------------------------------------------------
def dense32(spec, x, mel=None, lens=None, defect=None):
    W, b = spec["W"].to(F32), spec["b"].to(F32)
    a = x.to(F32)
    if spec["in_log"]:
        a = torch.log10(torch.clamp(a, min=1e-8)) * np.float32(spec["in_bn"][0]) + np.float32(spec["in_bn"][1])
    if spec["in_relu"]:
        a = torch.relu(a)
    if defect == "swap_rows":          # wT rows 40 and 41 = input channels 40 and 41 exchanged
        W = W.clone()
        W[:, [40, 41]] = W[:, [41, 40]]
    sc, sh = (np.float32(v) for v in (spec["out_bn"] or (1.0, 0.0)))
    v = a @ W.T
    if defect == "bias_after_bn":
        v = (torch.relu(v) if spec["out_relu"] else v) * sc + sh + b
    elif defect == "bn_before_relu":
        v = torch.relu((v + b) * sc + sh)
    else:
        v = v + b
        if spec["out_relu"]:
            v = torch.relu(v)
        v = v * sc + sh
    if spec["resid"]:
        v = v + (mel.to(F32) if defect == "linear_resid" else torch.log10(torch.clamp(mel.to(F32), min=1e-8)))
    return torch.where(R.live_mask(x.shape[0], x.shape[1], lens)[..., None], v, torch.zeros((), dtype=F32))


def gru32(sd, layer, xp, lens=None, defect=None):
    """k_gru_seq in fp32: xp (B, T, 1536), every row finite (a defect may read the rows past lens) -> y (B, T, 512)."""
    B, T, _ = xp.shape
    Whh, bhn = (t.to(F32) for t in R.gru_weights(sd, layer))
    if isinstance(defect, tuple) and defect[0] == "zero_col":
        Whh = Whh.clone()
        Whh[:, :, defect[1]] = 0.0
    if defect == "swap_cols":
        Whh = Whh.clone()
        Whh[:, :, [100, 101]] = Whh[:, :, [101, 100]]
    y = torch.zeros((B, T, 512), dtype=F32)
    for b in range(B):
        n = T if lens is None else lens[b]
        for d in range(2):
            order = list(range(n)) if d == 0 else list(range(n - 1, -1, -1))
            if defect == "backward_from_T" and d == 1:
                order = list(range(T - 1, -1, -1))
            h = torch.zeros(256, dtype=F32)
            for s, t in enumerate(order):
                x = xp[b, order[s - 1] if defect == "stale_x" and s > 0 else t, 768 * d:768 * (d + 1)].to(F32)
                g = Whh[d] @ h
                r = torch.sigmoid(x[:256] + g[:256])
                z = torch.sigmoid(x[256:512] + g[256:512])
                if defect == "swap_zr":
                    r, z = z, r
                if defect == "bhn_outside":
                    n_ = torch.tanh(x[512:] + bhn[d] + r * g[512:])
                else:
                    n_ = torch.tanh(x[512:] + r * (g[512:] + bhn[d]))
                h = n_ + z * (h - n_)
                if t < n:
                    y[b, t, 256 * d:256 * (d + 1)] = h
    if defect == "swap_halves":
        y = torch.cat([y[..., 256:], y[..., :256]], -1)
    return y


def _cases(piece):
    shapes = R.GRU_SHAPES if piece in R.GRU_PIECES else R.DENSE_SHAPES
    return shapes + ([R.CHUNK_SHAPE] if piece in R.CHUNK_PIECES else [])


def _run32(sd, piece, xs, lens, defect=None):
    if piece in R.GRU_PIECES:
        return gru32(sd, int(piece[3]), xs[0], lens, defect)
    return dense32(R.dense_spec(sd, piece), xs[0], xs[1] if len(xs) > 1 else None, lens, defect)


def _over_bar(sd, piece, xs, lens, got):
    """max |got - ref| / (D + 16 G) over the clips' elements, the reference reading NaN in the rows past lens."""
    ref, D, G = R.piece_ref(sd, piece, [R.nan_pad(x, lens) for x in xs], lens, got=got)
    return R.worst_over_bar(got, ref, D, G, R.K_CAP, lens)


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", ["bi_gru", "dnn"])
def test_piece_references_chain_to_the_module_restatement(sds, module):
    B, T, lens = R.CHAIN_SHAPE
    mel = R.mel_input(B, T, seed=41)
    for frames in (None, lens):
        want = reference_forward(module, sds[module], mel.numpy(), frames=frames)
        got = R.chain_ref(module, sds[module], R.nan_pad(mel, frames), frames).numpy()
        assert np.abs(got - want).max() < 1e-12, (module, frames, np.abs(got - want).max())


def test_heavy_weights_saturate_the_gates(sds):
    """The second weight set is what it claims: gates near 0 and 1 occur, and b_hn is large against W_hn h."""
    Whh, bhn = R.gru_weights(sds["heavy"], 0)
    Whh0, bhn0 = R.gru_weights(sds["bi_gru"], 0)
    assert torch.equal(Whh, 4 * Whh0) and torch.equal(bhn, 8 * bhn0)
    assert torch.equal(sds["heavy"]["2.gru.bias_hh_l0"][:512], sds["bi_gru"]["2.gru.bias_hh_l0"][:512])
    y = R.gru_free_ref(sds["heavy"], 0, R.rand_input(1, 40, 1536, seed=3, scale=4.0))
    assert y.abs().max() > 0.999


@pytest.mark.parametrize("piece", R.PIECES["bi_gru"] + R.PIECES["dnn"])
def test_fp32_evaluation_is_inside_the_bar(sds, piece):
    for heavy in ((False, True) if piece in R.GRU_PIECES else (False,)):
        sd = _sd_of(sds, piece, heavy)
        for scale in ((1.0, 4.0) if piece in R.GRU_PIECES else (1.0,)):
            for i, (B, T, lens) in enumerate(_cases(piece)):
                xs = R.piece_inputs(piece, B, T, seed=100 + i, scale=scale)
                worst = _over_bar(sd, piece, xs, lens, _run32(sd, piece, xs, lens))
                assert worst <= 1.0, (piece, heavy, scale, (B, T), worst)


DENSE_DEFECTS = [("lin1", "bias_after_bn"), ("fc1", "bias_after_bn"), ("fc0", "bn_before_relu"), ("fc2", "bn_before_relu"),
                 ("lin6", "linear_resid"), ("fc5", "linear_resid"), ("lin1", "swap_rows"), ("proj0", "swap_rows"),
                 ("proj1", "swap_rows"), ("lin4", "swap_rows"), ("fc3", "swap_rows")]


@pytest.mark.parametrize("piece,defect", DENSE_DEFECTS)
def test_planted_dense_defects_are_far_outside_the_bar(sds, piece, defect):
    sd = _sd_of(sds, piece)
    B, T, lens = R.DENSE_SHAPES[-1]
    xs = R.piece_inputs(piece, B, T, seed=7)
    assert _over_bar(sd, piece, xs, lens, _run32(sd, piece, xs, lens)) <= 1.0
    worst = _over_bar(sd, piece, xs, lens, _run32(sd, piece, xs, lens, defect))
    assert worst >= 100.0, (piece, defect, worst)


@pytest.mark.parametrize("piece", ["proj0", "proj1"])
@pytest.mark.parametrize("heavy", [False, True])
def test_projection_bias_without_b_hz_is_far_outside_the_bar(sds, piece, heavy):
    sd = _sd_of(sds, piece, heavy)
    B, T, lens = R.DENSE_SHAPES[-1]
    xs = R.piece_inputs(piece, B, T, seed=8)
    spec = R.dense_spec(sd, piece)
    for d, sfx in enumerate(("", "_reverse")):
        spec["b"][768 * d + 256:768 * d + 512] -= sd["2.gru.bias_hh_l%s%s" % (piece[4], sfx)][256:512].double()
    worst = _over_bar(sd, piece, xs, lens, dense32(spec, xs[0], None, lens))
    assert worst >= 100.0, (piece, worst)


# a column of each part of k_gru_seq's split of W_hh: registers [0, 120), LDS [120, 168), streamed [168, 256)
GRU_DEFECTS = [("zero_col", 60), ("zero_col", 140), ("zero_col", 200), "swap_cols", "stale_x", "bhn_outside", "swap_zr",
               "backward_from_T", "swap_halves"]


@pytest.mark.parametrize("defect", GRU_DEFECTS, ids=lambda d: d if isinstance(d, str) else "%s%d" % d)
@pytest.mark.parametrize("heavy", [False, True], ids=["synth", "heavy"])
@pytest.mark.parametrize("layer", [0, 1])
def test_planted_gru_defects_are_far_outside_the_bar(sds, layer, heavy, defect):
    sd = sds["heavy"] if heavy else sds["bi_gru"]
    piece = "gru%d" % layer
    B, T, lens = R.GRU_SHAPES[3]
    assert min(lens) < T
    xp = R.rand_input(B, T, 1536, seed=9)
    assert _over_bar(sd, piece, [xp], lens, gru32(sd, layer, xp, lens)) <= 1.0
    worst = _over_bar(sd, piece, [xp], lens, gru32(sd, layer, xp, lens, defect))
    assert worst >= 100.0, (piece, heavy, defect, worst)
