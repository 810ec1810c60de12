"""Shared by tests/test_gpu_analysis_launches.py and tests/test_analysis_f64_host.py: the float64 form of every launch of the bi_gru /
dnn analysis plans (csrc/analysis.hip: k_dense, k_gru_seq), the per-element bound a launch is held to, the seeded inputs and the shapes
of the cases.  A plain helper module, no tests.

Every reference is built from the PyTorch-layout state_dict (never from packed arrays: the transposition, the concatenation of the two
directions and the folding of b_hr / b_hz into the projection bias are part of what is tested) and takes the float32 values the launch
read, widened to float64.  With `lens`, clip b is its own first lens[b] rows; the reference is zero past them and input rows past them
are never looked at (the tests fill them with NaN).

A bound has two parts, bar = D + k * G (u32 = 2^-24, the unit roundoff of fp32):

D, derived.  k_dense (the structure of launch_parity_f64._bar, mode 0): a_i = the float64 value of the launch's input transform of
the fp32 input, w_i the fp32 weights, S = sum |a_i w_i|.
  * in-log transform a = fma(sc32, log10f(max(x, 1e-8)), sh32), sc32 / sh32 the fp32 roundings of the float64 BN scalars sc, sh:
    beside the error of log10f (G below) a differs from sc L + sh by at most u32 (|sc L| + |sh|) for the two rounded scalars plus
    u32 |a| for the fma: da_i <= 2 u32 (|sc L_i| + |sh|), which reaches the sum as sum da_i |w_i|.  ReLU and no transform are exact.
  * raw sum: K fmas and the bias addition round once each: (K + 2) u32 (S + |bias|).
  * ReLU: Lipschitz 1, the error passes unchanged.
  * output affine fma(sc32, v, sh32): |sc| e for the incoming error, u32 (|sc v| + |sh|) for the rounded scalars and as much for the
    fma's own rounding: |sc| e + 2 u32 (|sc v| + |sh|)  (the identity affine fma(1, v, 0) is exact; it is charged all the same).
  * residual v + log10f(.): one addition, 2 u32 (|v| + |L|) with the rounding of L to fp32.
k_gru_seq, ONE step: ref[t] is the float64 cell applied to the launch's own y[t -+ 1] (h = 0 at the clip's first step of either
direction), so the error does not accumulate over the sequence.  With g = W_hh h (four fma chains of 64 terms and three additions: at
most 258 u32 |W_hh| |h| =: eg per gate pre-activation), x the input projection and gn = g_n + b_hn:
  * r, z = 1 / (1 + expf(-(x + g))): the pre-activation carries eg + u32 |x + g| <= eg + 2 u32 (|x| + |g|) (the second u32 for the
    negation's operand being rounded already); sigmoid has Lipschitz constant 1/4; 1 + e and the result round once each, on values
    <= 1 relative to the result: e_r, e_z = (eg + 2 u32 (|x| + |g|)) / 4 + 2 u32.
  * n = tanhf(fma(r, fl(g_n + b_hn), x_n)): fl(g_n + b_hn) carries eg + u32 |gn|, the product |gn| e_r, the fma u32 (|x_n| + |gn|):
    e_n = eg + |gn| e_r + 3 u32 (|gn| + |x_n|)  (tanh: Lipschitz 1).
  * h' = fma(z, fl(h - n), n) = (1 - z) n + z h: e_n (1 - z) + |h - n| e_z, and u32 |h - n| + u32 |h'| <= 3 u32 (|h| + |n|) for the
    subtraction and the fma.
G, not derivable: the accuracy of the device's log10f, expf, tanhf and its division.  G = u32 times the magnitude through which an
error of one ulp of those results reaches the element: in-log sum |sc L_i| |w_i| (through the output affine: times |sc_out|);
residual |L|; a gate 1 through the gate's path, i.e. (|gn| + 1) (1 - z) + |h - n| for r, n and z together.  k is measured once on the
device and fixed in tests/test_gpu_analysis_launches.py; the CPU tests use the cap, k = 16."""
import numpy as np
import torch

U32 = 2.0 ** -24
K_CAP = 16.0

PIECES = {"bi_gru": ["lin1", "proj0", "gru0", "proj1", "gru1", "lin4", "lin6"], "dnn": ["fc0", "fc1", "fc2", "fc3", "fc4", "fc5"]}
# channels of the first input and of the output; lin6 / fc5 take the linear mel (128) as a second input
WIDTHS = {"lin1": (128, 256), "proj0": (256, 1536), "gru0": (1536, 512), "proj1": (512, 1536), "gru1": (1536, 512), "lin4": (512, 256),
          "lin6": (256, 128), "fc0": (128, 256), "fc1": (256, 512), "fc2": (512, 1024), "fc3": (1024, 512), "fc4": (512, 256),
          "fc5": (256, 128)}
MEL_IN = ("lin1", "fc0")          # the first input is the linear mel
MEL_RESID = ("lin6", "fc5")       # the second input is the linear mel
GRU_PIECES = ("gru0", "gru1")

# (B, T, lens).  k_dense works on M = B * T rows in tiles of 64: M = 1, 63, 64, 65 and 111 (clip boundaries inside a tile), then
# tiles that straddle a clip's end
DENSE_SHAPES = [(1, 1, None), (3, 21, None), (1, 64, None), (1, 65, None), (3, 37, None), (4, 90, [90, 61, 7, 1])]
# k_set_frames writes 64 frame counts per launch: chunks 2 and 3; 130 x 2 workgroups of k_gru_seq
CHUNK_SHAPE = (130, 3, [1 + b % 3 for b in range(130)])
CHUNK_PIECES = ("lin1", "fc0", "gru0")
# k_gru_seq: no prefetch; one prefetch; three steps; the backward start at T_b - 1 and zero rows; many steps
GRU_SHAPES = [(1, 1, None), (1, 2, None), (2, 3, None), (3, 37, [37, 20, 1]), (1, 300, None)]
CHAIN_SHAPE = (3, 37, [37, 20, 1])


def module_of(piece):
    return "dnn" if piece.startswith("fc") else "bi_gru"


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and weights
# ---------------------------------------------------------------------------------------------------------------------------------
def mel_input(B, T, seed):
    """Linear mel (B, T, 128) float32: log-uniform over 1e-7.5 .. 1e1.5 as the module tests', with exact zeros and values below the
    1e-8 clamp of to_log sprinkled in (every 7th, 11th and 13th element)."""
    rng = np.random.default_rng(seed)
    m = (10.0 ** rng.uniform(-7.5, 1.5, size=B * T * 128)).astype(np.float32)
    m[3::7] = 0.0
    m[5::11] = 1e-9
    m[2::13] = 3e-12
    return torch.from_numpy(m.reshape(B, T, 128))


def rand_input(B, T, C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, T, C), generator=g) * scale


def piece_inputs(piece, B, T, seed, scale=1.0):
    """The fp32 inputs of one case of `piece`: the mel where the launch takes one, randn (negatives included) elsewhere."""
    cin = WIDTHS[piece][0]
    xs = [mel_input(B, T, seed) if piece in MEL_IN else rand_input(B, T, cin, seed, scale)]
    if piece in MEL_RESID:
        xs.append(mel_input(B, T, seed + 1000))
    return xs


def live_mask(B, T, lens):
    if lens is None:
        return torch.ones((B, T), dtype=torch.bool)
    return torch.arange(T)[None, :] < torch.as_tensor(list(lens))[:, None]


def nan_pad(x, lens):
    """A copy of x (B, T, C) with NaN in the rows at and past lens[b]."""
    if lens is None:
        return x
    return torch.where(live_mask(x.shape[0], x.shape[1], lens)[..., None], x, torch.full_like(x, float("nan")))


def recurrence_heavy(sd):
    """A copy of the bi_gru state_dict with every weight_hh x 4 and the n third of every bias_hh x 8: the gates saturate and b_hn
    matters."""
    out = {k: v.clone() for k, v in sd.items()}
    for k in out:
        if ".weight_hh" in k:
            out[k] *= 4.0
        elif ".bias_hh" in k:
            out[k][512:] *= 8.0
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# k_dense
# ---------------------------------------------------------------------------------------------------------------------------------
def _bn(sd, p):
    g, b = sd[p + ".weight"].double()[0], sd[p + ".bias"].double()[0]
    mu, var = sd[p + ".running_mean"].double()[0], sd[p + ".running_var"].double()[0]
    sc = g / torch.sqrt(var + 1e-5)
    return float(sc), float(b - mu * sc)


def dense_spec(sd, piece):
    """What the launch `piece` computes, from the PyTorch-layout tensors: W (N, K), b (N) in float64, the input transform (in_log with
    its scalar BN, in_relu) and the epilogue (out_relu, the scalar BN, the to_log(mel) residual)."""
    s = dict(in_log=False, in_bn=(1.0, 0.0), in_relu=False, out_relu=False, out_bn=None, resid=False)
    if piece == "lin1":
        s.update(W=sd["1.weight"], b=sd["1.bias"], in_log=True, in_bn=_bn(sd, "0"), out_bn=_bn(sd, "2.bn"))
    elif piece in ("proj0", "proj1"):
        W, b = [], []
        for sfx in ("", "_reverse"):
            k = "_l%s%s" % (piece[4], sfx)
            W.append(sd["2.gru.weight_ih" + k])
            bh = sd["2.gru.bias_hh" + k].clone()
            bh[512:] = 0.0                     # b_hn stays inside r * (W_hn h + b_hn)
            b.append(sd["2.gru.bias_ih" + k].double() + bh.double())
        s.update(W=torch.cat(W), b=torch.cat(b))
    elif piece == "lin4":
        s.update(W=sd["4.weight"], b=sd["4.bias"], in_relu=True, out_relu=True)
    elif piece == "lin6":
        s.update(W=sd["6.weight"], b=sd["6.bias"], resid=True)
    else:
        i = int(piece[2])
        p = 3 * i if i < 5 else 14
        s.update(W=sd["%d.weight" % p], b=sd["%d.bias" % p], in_log=i == 0, out_relu=i < 5, resid=i == 5)
        if i < 4:
            s["out_bn"] = _bn(sd, str(p + 2))
    s["W"], s["b"] = s["W"].double(), s["b"].double()
    assert tuple(s["W"].shape) == WIDTHS[piece][::-1]
    return s


def to_log(mel):
    return torch.log10(torch.clamp(mel, min=1e-8))


def dense_ref(spec, x, mel=None, lens=None):
    """x (B, T, K) (and the linear mel of the residual): -> (ref, D, G), float64 (B, T, N); all three zero in the rows past lens."""
    B, T, K = x.shape
    live = live_mask(B, T, lens)[..., None]
    x = torch.where(live, x.double(), torch.ones((), dtype=torch.float64))
    W, b = spec["W"], spec["b"]
    Wa = W.abs().T
    a, da, ga = x, None, None
    if spec["in_log"]:
        sc, sh = spec["in_bn"]
        L = sc * to_log(x)
        a = L + sh
        da = 2 * U32 * (L.abs() + abs(sh))
        ga = U32 * L.abs()
    if spec["in_relu"]:
        a = torch.relu(a)
    v = a @ W.T + b
    e = (K + 2) * U32 * (a.abs() @ Wa + b.abs())
    g = torch.zeros_like(v)
    if da is not None:
        e = e + da @ Wa
        g = ga @ Wa
    if spec["out_relu"]:
        v = torch.relu(v)
    sc, sh = spec["out_bn"] or (1.0, 0.0)
    e = abs(sc) * e + 2 * U32 * ((sc * v).abs() + abs(sh))
    g = abs(sc) * g
    v = sc * v + sh
    if spec["resid"]:
        L = to_log(torch.where(live, mel.double(), torch.ones((), dtype=torch.float64)))
        e = e + 2 * U32 * (v.abs() + L.abs())
        g = g + U32 * L.abs()
        v = v + L
    z = torch.zeros((), dtype=torch.float64)
    return torch.where(live, v, z), torch.where(live, e, z), torch.where(live, g, z)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_gru_seq
# ---------------------------------------------------------------------------------------------------------------------------------
def gru_weights(sd, layer):
    """-> W_hh (2, 768, 256), b_hn (2, 256) of the forward and the backward direction, float64."""
    sfx = ["_l%d" % layer, "_l%d_reverse" % layer]
    return (torch.stack([sd["2.gru.weight_hh" + s].double() for s in sfx]),
            torch.stack([sd["2.gru.bias_hh" + s].double()[512:] for s in sfx]))


def _cell(xp, h, Whh, bhn):
    """One direction's cell: xp (.., 768) = W_i x + b_i (+ b_hr, b_hz), h (.., 256) -> h', and what the bound needs."""
    g = h @ Whh.T
    r = torch.sigmoid(xp[..., :256] + g[..., :256])
    z = torch.sigmoid(xp[..., 256:512] + g[..., 256:512])
    gn = g[..., 512:] + bhn
    n = torch.tanh(xp[..., 512:] + r * gn)
    return n + z * (h - n), (g, z, gn, n)


def _cell_bound(xp, h, Whh, bhn):
    hn, (g, z, gn, n) = _cell(xp, h, Whh, bhn)
    eg = 258 * U32 * (h.abs() @ Whh.abs().T)
    pre = 2 * U32 * (xp.abs() + g.abs())
    e_r = 0.25 * (eg[..., :256] + pre[..., :256]) + 2 * U32
    e_z = 0.25 * (eg[..., 256:512] + pre[..., 256:512]) + 2 * U32
    e_n = eg[..., 512:] + gn.abs() * e_r + 3 * U32 * (gn.abs() + xp[..., 512:].abs())
    D = e_n * (1 - z) + (h - n).abs() * e_z + 3 * U32 * (h.abs() + n.abs())
    G = U32 * ((gn.abs() + 1) * (1 - z) + (h - n).abs())
    return hn, D, G


def _previous(y, d, lens):
    """y (B, T, 256) of direction d -> the state each step started from: y[t - 1] forward, y[t + 1] backward, zero at the clip's first
    step (t = 0; t = lens[b] - 1)."""
    B, T, _ = y.shape
    zero = torch.zeros((B, 1, 256), dtype=y.dtype)
    if d == 0:
        return torch.cat([zero, y[:, :-1]], 1)
    hp = torch.cat([y[:, 1:], zero], 1)
    for b in range(B):
        hp[b, (T if lens is None else lens[b]) - 1] = 0.0
    return hp


def gru_step_ref(sd, layer, xp, y, lens=None):
    """The one-step reference of a k_gru_seq launch: xp (B, T, 1536) its input, y (B, T, 512) ITS OWN output -> (ref, D, G)."""
    B, T, _ = xp.shape
    live = live_mask(B, T, lens)[..., None]
    z = torch.zeros((), dtype=torch.float64)
    xp = torch.where(live, xp.double(), z)
    y = torch.where(live, y.double(), z)
    Whh, bhn = gru_weights(sd, layer)
    out = []
    for d in range(2):
        out.append(_cell_bound(xp[..., 768 * d:768 * (d + 1)], _previous(y[..., 256 * d:256 * (d + 1)], d, lens), Whh[d], bhn[d]))
    return tuple(torch.where(live, torch.cat([o[i] for o in out], -1), z) for i in range(3))


def gru_free_ref(sd, layer, xp, lens=None):
    """The layer run freely in float64 (the chaining test): xp (B, T, 1536) -> (B, T, 512), zero past lens."""
    B, T, _ = xp.shape
    Whh, bhn = gru_weights(sd, layer)
    y = torch.zeros((B, T, 512), dtype=torch.float64)
    for b in range(B):
        n = T if lens is None else lens[b]
        for d in range(2):
            h = torch.zeros(256, dtype=torch.float64)
            for t in (range(n) if d == 0 else range(n - 1, -1, -1)):
                h, _ = _cell(xp[b, t, 768 * d:768 * (d + 1)].double(), h, Whh[d], bhn[d])
                y[b, t, 256 * d:256 * (d + 1)] = h
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# one piece; the chain; the check
# ---------------------------------------------------------------------------------------------------------------------------------
def piece_ref(sd, piece, inputs, lens=None, got=None):
    """(ref, D, G) of one launch on its fp32 inputs.  The GRU pieces are one-step references: they need `got`, the launch's output."""
    if piece in GRU_PIECES:
        return gru_step_ref(sd, int(piece[3]), inputs[0], got, lens)
    return dense_ref(dense_spec(sd, piece), inputs[0], inputs[1] if len(inputs) > 1 else None, lens)


def chain_ref(module, sd, mel, lens=None):
    """The piece references fed into each other in float64, nothing rounded in between: mel (B, T, 128) -> log-mel (B, T, 128)."""
    mel = torch.as_tensor(np.asarray(mel)).double()
    h = mel
    for piece in PIECES[module]:
        if piece in GRU_PIECES:
            h = gru_free_ref(sd, int(piece[3]), h, lens)
        else:
            h = dense_ref(dense_spec(sd, piece), h, mel if piece in MEL_RESID else None, lens)[0]
    return h


def compare(got, ref, D, G, lens=None):
    """-> (worst |err| / D over the elements without G, the smallest k with |err| <= D + k G over those with G -- 0 where D alone
    suffices --, worst |err|).  Asserts that the live rows are finite and the rows past lens exactly 0.0."""
    got = got.detach().cpu().double()
    live = live_mask(got.shape[0], got.shape[1], lens)
    assert torch.isfinite(got[live]).all(), "non-finite values inside the clips"
    assert (got[~live] == 0).all(), "rows past a clip's frames are not exactly 0.0"
    err = (got - ref).abs()[live]
    D, G = D[live], G[live]
    assert (D > 0).all()
    plain = G == 0
    ratio = float((err[plain] / D[plain]).max()) if plain.any() else 0.0
    k = float(((err[~plain] - D[~plain]) / G[~plain]).clamp(min=0).max()) if (~plain).any() else 0.0
    return ratio, k, float(err.max())


def worst_over_bar(got, ref, D, G, k, lens=None):
    """max |err| / (D + k G) over the live elements."""
    got = got.detach().cpu().double()
    live = live_mask(got.shape[0], got.shape[1], lens)
    return float(((got - ref).abs()[live] / (D + k * G)[live]).max())
