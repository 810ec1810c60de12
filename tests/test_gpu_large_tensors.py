"""GPU: launches on tensors in the upper half of the 32-bit byte-offset range -- above 2^31 bytes, below the 2^32 - 4096 the planner
refuses (tests/large_cases.py: the case table and why these sizes).

Every case goes through the debug ops on one-launch plans (op_unet_piece, op_voc_resblock, op_voc_conv1d, op_voc_upsample,
op_voc_final).  P = 2 clips are drawn on the host exactly as the small-size launch tests draw them, uploaded, and repeated on the device to
B clips: clip b holds pattern b mod P.  Three checks:

  1. clips 0 and 1 of the large launch lie inside the float64 per-element bound the family is held to at small sizes -- the case
     helpers of tests/test_gpu_resunet_launches.py and tests/test_gpu_vocoder_launches.py and the reference of tests/resstack_f64.py
     run unchanged, with the large launch standing in for the small one (`run`);
  2. every clip b >= P equals clip b - P of the same output bit for bit (hence clip b mod P), compared on the device as integers,
     bytes the op leaves untouched included: it is one launch, the same tiling per image, the same split-K factor, and the kernels
     are deterministic.  Read off the kernels: the image index enters k_conv, k_resblock and k_block2d32 only through the base
     offset img * img_stride of a tile's addresses (conv.hip set_origin / otab, resblock.hip otab), the small kernels and the tail
     only through b * stride -- no family's arithmetic depends on the clip index, so none is exempted;
  3. tests/test_large_tensors_host.py: the byte counts, where byte 2^31 falls, and the planner's choice of family, by arithmetic.

The negative control flips one bit in the last clip of a passing output and requires the comparison of check 2 to name that clip.

Memory: an op copies the caller's tensors into its plan's arena and back, and op_unet_piece also returns the tensor between two
launches, so a case holds up to eight tensors of 2.7 GB on the device (NEED); a case skips only where less than that is free."""
import pytest
import torch

import large_cases as LC
import resstack_f64 as RS
import test_gpu_resunet_launches as L
import test_gpu_vocoder_launches as V
from conftest import TOL
from launch_parity_f64 import _check

pytestmark = pytest.mark.gpu

P = LC.P
NEED = 24 << 30   # bytes of device memory a case may hold: eight tensors of 2.7 GB and the comparison's temporaries


def _ids(cases):
    return [c.name for c in cases]


@pytest.fixture(scope="module")
def sds():
    from voicefixer_main_amd import synth
    return {"mel": synth.make_resunet_state_dict(0), "spec": synth.make_resunet_state_dict(2)}


@pytest.fixture(scope="module")
def engines(sds):
    """get(precision): a handle with both ResUNets' synthetic weights (the vocoder ops take their weights as arguments)."""
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_UNET_SPEC
    made = {}

    def get(precision):
        if precision not in made:
            eng = Engine("cuda:0", config={"precision": precision})
            eng.load_state_dict(MODEL_UNET_MEL, sds["mel"])
            eng.load_state_dict(MODEL_UNET_SPEC, sds["spec"])
            eng.tol = TOL[precision]
            made[precision] = eng
        return made[precision]
    yield get
    for eng in made.values():
        eng.close()


@pytest.fixture(autouse=True)
def _room():
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < NEED:
        pytest.skip("%d bytes of device memory are free, the case needs %d" % (free, NEED))
    yield
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------------
# the periodic batch and its comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def mismatched_clips(t):
    """t (B, ...) on the device -> the clips b >= P whose bits differ from clip b - P, a few clips' worth of temporaries at a time."""
    bits = _bits(t).reshape(t.shape[0], -1)
    step = max(1, (1 << 27) // bits.shape[1])
    bad = []
    for b in range(P, t.shape[0], step):
        e = min(t.shape[0], b + step)
        ne = (bits[b:e] != bits[b - P:e - P]).any(dim=1)
        bad += [b + int(i) for i in ne.nonzero().flatten().tolist()]
    return bad


class Periodic:
    """Stands in for an op of the engine: every activation tensor of P clips among the arguments is repeated on the device to B
    clips, the op runs once on those, every output of B clips is held to check 2 and handed back cut to its first P clips."""

    def __init__(self, op, B, keep=False):
        assert B % P == 0
        self.op, self.B, self.keep, self.checked, self.kept = op, B, keep, [], None

    def _grow(self, a):
        if isinstance(a, torch.Tensor) and a.dim() >= 2 and a.shape[0] == P:
            return a.to("cuda").repeat((self.B // P,) + (1,) * (a.dim() - 1))
        if isinstance(a, list):
            return [self._grow(v) for v in a]
        return a

    def _cut(self, r):
        if isinstance(r, torch.Tensor) and r.dim() >= 1 and r.shape[0] == self.B:
            bad = mismatched_clips(r)
            assert not bad, ("clips that differ from the clip %d in front of them" % P, bad[:8], len(bad), tuple(r.shape))
            self.checked.append((tuple(r.shape), r.numel() * r.element_size()))
            if self.keep and (self.kept is None or r.numel() >= self.kept.numel()):
                self.kept = r
            return r[:P].clone()
        if isinstance(r, (tuple, list)):
            return type(r)(self._cut(v) for v in r)
        return r

    def __call__(self, *args, **kw):
        out = self.op(*[self._grow(a) for a in args], **{k: self._grow(v) for k, v in kw.items()})
        return self._cut(out)


def _covers(run, case):
    """The launch did run at the case's size: an output (or the tensor between two launches) of B clips was compared, and the
    largest tensor of the case lies in (2^31, 2^32 - 4096) bytes."""
    assert run.checked and LC.LO < case.nbytes < LC.HI, (case.name, run.checked, case.nbytes)
    assert all(shape[0] == case.B for shape, _ in run.checked), run.checked


# ---------------------------------------------------------------------------------------------------------------------------------
# ResUNet pieces
# ---------------------------------------------------------------------------------------------------------------------------------
def _unet_case(engines, sds, case, keep=False):
    from voicefixer_main_amd.engine import MODEL_UNET_MEL, MODEL_UNET_SPEC
    a = case.args
    eng, sd = engines(a["precision"]), sds[a["model"]]
    model = {"mel": MODEL_UNET_MEL, "spec": MODEL_UNET_SPEC}[a["model"]]
    run = Periodic(eng.op_unet_piece, case.B, keep)
    piece, (H, W) = a["piece"], a["hw"]
    if piece == "entry":
        fam = L._entry_case(eng, sd, H, W, model, B=P, run=run)
    elif piece == "pool":
        L._pool_case(eng, H, W, case.large[-1], model, run=run)
        fam = ["small"]
    elif piece == "final":
        fam = L._final_spec_case(eng, sd, H - 3, W, model, run=run)   # rows < T = 61 of the Tpad = 64 trunk
    elif piece.endswith(".up"):
        fam = L._up_case(eng, sd, int(piece[3]), H, W, True, 77, model, run=run)
    else:
        (launches,) = L._block_case(eng, sd, piece, H, W, 78, model=model, B=P, run=run, plan_B=case.B)
        fam = L._families(launches)
    assert fam == a["families"], (case.name, fam)
    _covers(run, case)
    return run


@pytest.mark.parametrize("case", LC.UNET_CASES, ids=_ids(LC.UNET_CASES))
def test_unet_piece(engines, sds, case):
    """Level 1 of the spectrogram model at B = 320 (entry, the C = 32 identity block on k_block2d32 and as two fp32 k_conv launches,
    dec6.1's two sources, after, pool, the two-output epilogue, dec6's pruned upsampler into the large tensor), enc2.2 at B = 640
    (k_resblock G2), enc3.2 at B = 1280 (k_conv, C = 128), and the mel model's level 1 and level 3 blocks, where a clip straddles
    byte 2^31 inside a tile."""
    _unet_case(engines, sds, case)


# ---------------------------------------------------------------------------------------------------------------------------------
# vocoder launches, fp32 trunk
# ---------------------------------------------------------------------------------------------------------------------------------
def _voc(cases, kind):
    return [c for c in cases if c.kind == kind]


@pytest.mark.parametrize("case", _voc(LC.VOC_CASES, "voc_resblock"), ids=_ids(_voc(LC.VOC_CASES, "voc_resblock")))
def test_voc_resblock(engines, case):
    """One fused ResStack layer on the fp32 trunk (k_resblock, split-bf16), an unfolded and a folded dilation, C = 64 and 128: the
    reference and bar of tests/test_gpu_resstack_launches.py's bf16 forms (raw fp32 output)."""
    a = case.args
    eng = engines(a["precision"])
    T, C = case.large
    x = RS.random_trunk(P, T, C, 9000 + C + a["dil"])
    layer = RS.random_layer(C, 9100 + C + a["dil"])
    run = Periodic(eng.op_voc_resblock, case.B)
    eng.take_flags()
    y, ya, info = run(x, layer, a["dil"], slope=V.RES_SLOPE, act_slope=V.UP_SLOPE, want_raw=True, want_act=False)
    assert eng.take_flags() == 0 and ya is None
    assert (info["rw"], info["r128"], info["asrc"], info["x16"], info["fold"]) == (0, 0, 0, 0, a["fold"]), info
    for b in range(P):
        ref = RS.resstack_ref(x[b], [layer], [a["dil"]], V.RES_SLOPE, V.UP_SLOPE, a["precision"], eng.tol["conv"])
        _check(y[b].cpu(), ref["y"], ref["bar_y32"], (case.name, b))
    _covers(run, case)


@pytest.mark.parametrize("case", _voc(LC.VOC_CASES, "voc_conv1d"), ids=_ids(_voc(LC.VOC_CASES, "voc_conv1d")))
def test_voc_conv1d(engines, case):
    """Conv1d 128 -> 128 k3 on plain k_conv, fp32 and split-bf16, d = 1 and a folded dilation: the raw fp32 source through the launch's
    LeakyReLU prologue, a raw residual, a raw output -- source, residual and output are all large."""
    a = case.args
    eng = engines(a["precision"])
    T, C = case.large
    run = Periodic(eng.op_voc_conv1d, case.B)
    V._conv_case(eng, a["precision"], C, C, T, P, 3, a["dil"], 9200 + a["dil"], act=1, slope=V.RES_SLOPE, residual=True, run=run)
    assert not eng.last_conv_w64
    _covers(run, case)


def test_voc_upsample(engines):
    """A x4 upsampler 128 -> 64 (phased k_conv, raw source, raw output) whose output is the large tensor."""
    case = LC.by_name("upsample-x4")
    a = case.args
    eng = engines(a["precision"])
    run = Periodic(eng.op_voc_upsample, case.B)
    assert not V._run_upsample(eng, a["precision"], a["Cin"], a["stride"], a["T"], P, 9300, False, "raw", None, run=run)
    _covers(run, case)


def test_voc_final(engines):
    """The tail on a large fp32 trunk (one block row per clip, 64-bit clip offsets)."""
    case = LC.by_name("final-c64")
    eng = engines(case.args["precision"])
    T, C = case.large
    run = Periodic(eng.op_voc_final, case.B)
    V._final_case(eng, P, T, C, None, False, 9400, run=run)
    assert run.checked and LC.LO < case.nbytes < LC.HI   # (the output is (B, T): the SOURCE is the large tensor)


# ---------------------------------------------------------------------------------------------------------------------------------
# just over the limit: the planner refuses on the host, nothing is launched
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,piece,B,hw,precision,err", LC.REFUSED_UNET, ids=[r[0] for r in LC.REFUSED_UNET])
def test_refused_at_4gib(engines, what, piece, B, hw, precision, err):
    """The smallest batch whose tensor reaches 2^32 - 4096 bytes: op_unet_piece returns the library's error from the plan builder's
    host checks, before any copy or launch (the inputs are uninitialised memory that nothing reads)."""
    from voicefixer_main_amd.engine import MODEL_UNET_SPEC
    eng = engines(precision)
    C = {"enc1.2": 32, "enc2.2": 64, "enc3.2": 128}[piece]
    assert B * hw[0] * hw[1] * C * 4 >= LC.HI > (B - 1) * hw[0] * hw[1] * C * 4
    x = torch.empty((B,) + tuple(hw) + (C,), device="cuda")
    eng.take_flags()
    with pytest.raises(RuntimeError, match=err):
        eng.op_unet_piece(piece, [x], model=MODEL_UNET_SPEC)
    assert eng.take_flags() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# negative control
# ---------------------------------------------------------------------------------------------------------------------------------
def test_comparison_sees_the_last_clip(engines, sds):
    """One bit flipped in the last element of the last clip of a passing large output -- its highest address -- and one in the
    clip that starts at byte 2^31: the comparison of check 2 names exactly those clips."""
    case = LC.by_name("dec6.up")
    y = _unet_case(engines, sds, case, keep=True).kept
    assert y.shape[0] == case.B and y.numel() * 4 == case.nbytes and mismatched_clips(y) == []
    flat = _bits(y).reshape(case.B, -1)
    flat[case.B - 1, -1] ^= 1
    assert mismatched_clips(y) == [case.B - 1]
    b = case.straddle()[0]
    flat[b, 0] ^= 1 << 30
    assert mismatched_clips(y) == [b, b + P, case.B - 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# a whole call at the largest batch Engine.vocoder keeps in one launch
# ---------------------------------------------------------------------------------------------------------------------------------
def _voc_bytes_per_frame(cfg):
    """COPIED (api.cpp max_clips_per_launch): the bytes one conditioning frame takes in the vocoder's widest-in-bytes fp32 tensor --
    the input of the first upsampler, or the output of a stage (channels halve, positions grow by the stage's scale)."""
    c, mul, widest = int(cfg.voc_channels), 1, int(cfg.voc_channels) * 4
    for i in range(int(cfg.voc_n_stages)):
        mul *= int(cfg.voc_scales[i])
        c //= 2
        widest = max(widest, mul * c * 4)
    return widest


def test_vocoder_call_at_the_largest_single_launch(voc_sd):
    """Engine.vocoder in split-bf16 (every trunk fp32) at B = the largest count max_clips_per_launch keeps in ONE launch, 2^32 - 2^20
    bytes over the widest stack's bytes per clip: that stack then lies within one clip of 4 GiB.  The mel is clip-periodic: rows
    b >= P equal rows b - P bit for bit, rows 0 and 1 equal the B = 2 call's, and no device flag is raised.  T comes from the
    handle's layer table: the frame count at which about 512 clips fill the range."""
    import numpy as np
    from voicefixer_main_amd.engine import Engine, MODEL_VOCODER
    eng = Engine("cuda:0", config={"precision": 1})
    eng.load_state_dict(MODEL_VOCODER, voc_sd)
    per_frame = _voc_bytes_per_frame(eng.cfg)
    lim = (1 << 32) - (1 << 20)
    T = lim // (512 * per_frame) - 4
    T -= T % 2
    per_clip = (T + 4) * per_frame
    B = lim // per_clip
    B -= B % P                       # (clip-periodic; still more than 2 GiB)
    assert T >= 8 and LC.LO < B * per_clip <= lim and (B + P) * per_clip > lim, (T, B, per_clip)
    rng = np.random.default_rng(17)
    mel = torch.from_numpy((10.0 ** (rng.normal(size=(P, T, 128)) * 1.2 - 2.5)).astype(np.float32)).cuda()
    eng.take_flags()
    small = eng.vocoder(mel)
    big = eng.vocoder(mel.repeat(B // P, 1, 1))
    assert eng.take_flags() == 0
    assert big.shape == (B, eng.vocoder_out_len(T)) and bool(torch.isfinite(big).all())
    assert mismatched_clips(big) == []
    assert torch.equal(_bits(big[:P]), _bits(small))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the vocoder ops just over 4 GiB - 4096, and the 16-bit families at their own limit of 2^31
# ---------------------------------------------------------------------------------------------------------------------------------
def test_voc_ops_refused_at_4gib(engines):
    """A trunk of exactly 2^32 bytes: the fused layer (plan_resblock) and the plain convolution (finish_params) return the library's
    error from their host checks; nothing was launched, no flag is raised, and the handle still runs the next launch."""
    eng = engines(1)
    eng.take_flags()
    layer = RS.random_layer(64, 1)
    x = torch.empty((512, 1 << 15, 64), device="cuda")
    assert x.numel() * 4 >= LC.HI
    with pytest.raises(RuntimeError, match="resblock: tensor exceeds 4 GiB"):
        eng.op_voc_resblock(x, layer, 1, slope=V.RES_SLOPE, act_slope=V.UP_SLOPE)
    del x
    x = torch.empty((256, 1 << 15, 128), device="cuda")
    w, b = V._rand((128, 128, 3), 2, 0.05), V._rand((128,), 3, 0.1)
    with pytest.raises(RuntimeError, match="exceeds 4 GiB"):
        eng.op_voc_conv1d(x, w.numpy(), b.numpy(), act=1, slope=V.RES_SLOPE)
    del x
    assert eng.take_flags() == 0
    V._conv_case(eng, 1, 128, 128, 130, 1, 3, 1, 9500, act=1, slope=V.RES_SLOPE)


W64_B, W64_C = 512, 256          # k_resblock_w64 checks B T C x 4 bytes (an fp32 trunk's) against 2^31
W64_T_UNDER, W64_T_OVER = (1 << 12) - 3, 1 << 12


def test_resblock_w64_below_its_limit():
    """The wide 16-bit layer (C = 256: resblock_w64.hip, activated fp16 trunk in, activated fp16 out) 1.5 MB below its limit of
    B T C x 4 < 2^31, an unfolded and a folded dilation: the reference and bar of the w64-c256 form of
    tests/test_gpu_resstack_launches.py.  The trunk crosses the call as the fp16 device tensor the launch in front would store."""
    from voicefixer_main_amd.engine import Engine
    eng = Engine("cuda:0", config={"precision": 2})
    B, T, C = W64_B, W64_T_UNDER, W64_C
    assert LC.LIMIT16 - (3 << 20) < B * T * C * 4 < LC.LIMIT16
    x = RS.random_trunk(P, T, C, 9600)
    xa = torch.nn.functional.leaky_relu(x, V.RES_SLOPE).half()     # resstack_ref's xa = fp16(LeakyReLU32(x))
    for dil in (1, LC.FOLDED):
        layer = RS.random_layer(C, 9610 + dil)
        run = Periodic(lambda xa_, **kw: eng.op_voc_resblock_at(None, xa_, layer, dil, **kw), B)
        eng.take_flags()
        y, ya, info = run(xa, slope=V.RES_SLOPE, act_slope=V.RES_SLOPE, want_raw=False, want_act=True)
        assert eng.take_flags() == 0 and y is None
        assert (info["asrc"], info["x16"], info["rw"], info["r128"]) == (1, 1, 0, 0), info
        for b in range(P):
            ref = RS.resstack_ref(x[b], [layer], [dil], V.RES_SLOPE, V.RES_SLOPE, 2, TOL[2]["conv"], x16=True, asrc=True)
            _check(ya[b].cpu(), ref["ya"], ref["bar_ya"], ("w64", dil, b))
        assert run.checked == [((B, T, C), B * T * C * 4)]          # (ya comes back widened to fp32)
    eng.close()


def test_resblock_w64_refused_at_its_limit():
    """B T C x 4 = 2^31 exactly: the fused kernel refuses with its error and launches nothing."""
    from voicefixer_main_amd.engine import Engine
    eng = Engine("cuda:0", config={"precision": 2})
    assert W64_B * W64_T_OVER * W64_C * 4 == LC.LIMIT16
    xa = torch.zeros((W64_B, W64_T_OVER, W64_C), device="cuda", dtype=torch.float16)
    with pytest.raises(RuntimeError, match="resblock_w64: tensor exceeds 2 GiB"):
        eng.op_voc_resblock_at(None, xa, RS.random_layer(W64_C, 1), 1, slope=V.RES_SLOPE, act_slope=V.RES_SLOPE, want_raw=False, want_act=True)
    assert eng.take_flags() == 0
    eng.close()


CW64_B, CW64_C = 1024, 512       # conv_w64_ok: B T Cin x 2 and B T Cout x 2 bytes (the fp16 tensors') below 2^31


@pytest.mark.parametrize("T,w64", [((1 << 11) - 1, True), (1 << 11, False), (5 << 9, False)], ids=["under", "at", "upper-half"])
def test_conv_w64_at_its_limit(T, w64):
    """conv1 of a C = 512 layer (activated fp16 source and output, as stored) 1 MB below k_conv_w64's limit of 2^31 bytes per tensor
    -- the launch runs on k_conv_w64 --, with tensors of exactly 2^31 bytes, where the plan falls back to k_conv, and with fp16
    tensors of 2.7 GB on k_conv, in the upper half of its offsets: all inside the float64 bound of tests/test_gpu_conv_w64.py's
    test_vs_fp64 and clip-periodic, d = 1 and a folded dilation.  (finish_params counted an activated fp16 source at four bytes an
    element and refused the fallback at half of k_conv's range; it now counts the bytes build_stages gives the descriptor.)"""
    import numpy as np
    import torch.nn.functional as F
    from launch_parity_f64 import _act64, _act_bar, _bar, _operand
    from voicefixer_main_amd.engine import Engine
    eng = Engine("cuda:0", config={"precision": 2})
    B, C = CW64_B, CW64_C
    assert (B * T * C * 2 < LC.LIMIT16) == w64 and B * T * C * 2 > LC.LIMIT16 - (2 << 20)
    x = F.leaky_relu(V._rand((P, T, C), 9700), V.RES_SLOPE).half()
    w = V._rand((C, C, 3), 9701, 1.0 / np.sqrt(3 * C))
    b = V._rand((C,), 9702, 0.1)
    wq = _operand(w, 2)
    run = Periodic(eng.op_voc_conv1d, B)
    eng.take_flags()
    for dil in (1, 27):
        y, ya = run(x.cuda(), w.numpy(), b.numpy(), dil=dil, src_act=True, act=1, slope=V.RES_SLOPE, want_raw=False, next_act=1,
                    next_slope=V.RES_SLOPE, stored=True)
        assert y is None and ya.dtype == torch.float16 and eng.last_conv_w64 == w64, (dil, eng.last_conv_w64)
        for bi in range(P):
            a = x[bi:bi + 1].double().permute(0, 2, 1)
            ref = F.conv1d(a, wq, b.double(), padding=dil, dilation=dil)[0].T
            S = F.conv1d(a.abs(), wq.abs(), padding=dil, dilation=dil)[0].T
            bar, cap = _bar(ref, S, 3 * C, 2, TOL[2]["conv"], extra=b.double().abs()[None, :])
            ra = _act64(ref, 1, V.RES_SLOPE)
            _check(ya[bi].cpu().float(), ra, _act_bar(ra, bar, V.RES_SLOPE, 2, cap), ("conv_w64", T, dil, bi))
    assert eng.take_flags() == 0
    assert run.checked == [((B, T, C), B * T * C * 2)] * 2
    eng.close()
