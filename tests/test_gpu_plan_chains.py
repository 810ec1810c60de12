"""Every whole plan equals the chain of its own launches, bit for bit (tests/plan_chains.py).

The launch tests hold each launch of the ResUNets and of the vocoder to float64 on operands of its own; the model tests hold the whole
calls to the oracle within bars a whole network's rounding passes.  Here the two meet: Engine.resunet_mel, resunet_spec, vocoder and
restore_gsr against the one-launch plans of the test library run one behind the other, wired the way the NETWORK is wired
(oracle/resunet.py, oracle/vocoder.py), not the way the plan builders are written.  The kernels are deterministic
and both sides build a launch with the same builder functions, so the bar is torch.equal: what differs is the plan -- a wrong source
buffer, skip order, tensor form, slope, packing mode, split-K rule, or two live tensors on the same bytes of the arena (each one-launch
plan has buffers of its own; the whole plan shares one first-fit arena).  The negative controls at the end say the equalities bite.

tests/test_plan_chains_host.py holds the whole plans' launch lists to the chain's on the host: the chain here IS the plan's launches.
"""
import numpy as np
import pytest
import torch

import plan_chains as PC
from conftest import TOL

pytestmark = pytest.mark.gpu

MEL_SHAPES = [(1, 1), (2, 64), (3, 65), (2, 130), (1, 1990)]     # Tpad 64, 64, 128, 192, 2048: the three short_clip classes
# (1, 3): the fewest frames a clip that the STFT's reflect padding accepts can have (n_fft / 2 < L); one padded chunk as T = 1 would be
SPEC_SHAPES = [(1, 3), (2, 70), (1, 130)]
VOC_SHAPES = [(1, 1), (2, 2), (2, 21)]


def _mel_input(B, T, seed=0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((10.0 ** (rng.normal(size=(B, T, 128)) * 1.2 - 2.5)).astype(np.float32)).cuda()


def _engine(precision, tuning, models, cfg=None):
    """A handle with a tuning word / layer table of its own; models: {model: state dict}."""
    from voicefixer_main_amd.engine import Engine
    eng = Engine("cuda:0", config=dict({"precision": precision, "tuning": tuning}, **(cfg or {})))
    for model, sd in models.items():
        eng.load_state_dict(model, sd)
    eng.tol = TOL[precision]
    return eng


def _same(a, b, what):
    assert a.shape == b.shape and bool(torch.isfinite(a).all()), what
    assert torch.equal(a, b), (what, "%d of %d elements differ, max %g" % (int((a != b).sum()), a.numel(), float((a - b).abs().max())))


def _differ(a, b, what):
    assert a.shape == b.shape, what
    frac = float((a != b).float().mean())
    assert frac > 0.01, (what, "only %.4f of the elements differ" % frac)


# ---------------------------------------------------------------------------------------------------------------------------------
# ResUNets
# ---------------------------------------------------------------------------------------------------------------------------------
def _mel_case(eng, B, T):
    from voicefixer_main_amd.engine import MODEL_UNET_MEL
    mel = _mel_input(B, T, seed=T)
    eng.take_flags()
    whole = eng.resunet_mel(mel)
    assert eng.take_flags() == 0
    (chain,) = PC.unet_chain(eng, MODEL_UNET_MEL, mel, [mel])
    assert eng.take_flags() == 0
    _same(whole, chain, ("resunet_mel", eng.tol["name"], eng.cfg.tuning, B, T))


@pytest.mark.parametrize("B,T", MEL_SHAPES)
def test_resunet_mel_is_its_chain(engine, B, T):
    """prep_logmel, entry, the encoders with their pools, the bottleneck, the decoders on (upsampled, skip of level 7 - d), after and
    final, every piece with the short_clip the documented rule gives this Tpad: the whole call's bits."""
    assert PC.short_clip_of((T + 63) // 64 * 64) == {1: 1, 64: 1, 65: 1, 130: 0, 1990: -2}[T]
    _mel_case(engine, B, T)


@pytest.mark.parametrize("tuning", ["DEBUG_POISON_ARENA", "OLD_BLOCK2D", "TWO_LAUNCH_UPSAMPLERS"])
def test_resunet_mel_is_its_chain_under_tuning(unet_sd, tuning):
    """The arena re-poisoned before every plan run; the level-1 blocks on k_resblock's 16 x 16 tiles; two launches per upsampler."""
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import MODEL_UNET_MEL
    eng = _engine(1, getattr(_lib, "TUNE_" + tuning), {MODEL_UNET_MEL: unet_sd})
    for B, T in MEL_SHAPES:
        _mel_case(eng, B, T)
    eng.close()


@pytest.fixture(scope="module")
def spec_engines():
    """One handle per arithmetic mode with the spectrogram ResUNet, the synthetic weights of test_gpu_models.spec_engines."""
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.engine import MODEL_UNET_SPEC
    sd = synth.make_resunet_state_dict(2)
    engines = {}

    def get(precision):
        if precision not in engines:
            engines[precision] = _engine(precision, 0, {MODEL_UNET_SPEC: sd})
        return engines[precision]
    yield get
    for eng in engines.values():
        eng.close()


@pytest.mark.parametrize("B,T", SPEC_SHAPES)
def test_resunet_spec_is_its_chain(engine, spec_engines, B, T):
    """op_stft (sp, cos, sin), prep_spec, the trunk at width 1024 with pruned upsamplers, final (re, im), op_istft."""
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.engine import MODEL_UNET_SPEC
    eng = spec_engines(engine.precision)
    L = (T - 1) * eng.hop + 400
    assert eng.frames(L) == T
    wav = torch.from_numpy(synth.make_clips(B, L / 44100.0 + 0.01, seed=60 + T)[:, 0, :L].copy()).cuda()
    f = eng.op_stft(wav, want=("sp", "cos", "sin"))
    eng.take_flags()
    whole = eng.resunet_spec(f["sp"], wav)
    assert eng.take_flags() == 0
    re, im = PC.unet_chain(eng, MODEL_UNET_SPEC, f["sp"], [f["cos"], f["sin"]])
    chain = eng.op_istft(re, im, L)
    assert eng.take_flags() == 0
    _same(whole, chain, ("resunet_spec", eng.tol["name"], B, T))


# ---------------------------------------------------------------------------------------------------------------------------------
# vocoder
# ---------------------------------------------------------------------------------------------------------------------------------
def _voc_case(eng, sd, B, T, **controls):
    mel = _mel_input(B, T, seed=100 + T)
    eng.take_flags()
    whole = eng.vocoder(mel)
    wf = eng.take_flags()
    log = []
    chain = PC.vocoder_chain(eng, sd, mel, log=log, **controls)
    cf = eng.take_flags()
    return whole, chain, wf, cf, log


@pytest.mark.parametrize("B,T", VOC_SHAPES)
def test_vocoder_is_its_chain(engine, voc_sd, B, T):
    """voc_prep, the condnet, the k7 reflect convolution, per stage an upsampler and its ResStack, the tail: every tensor in the form
    its consumer reads, handed over as its producer stored it."""
    whole, chain, wf, cf, log = _voc_case(engine, voc_sd, B, T)
    assert wf == cf == 0, (wf, cf)
    _same(whole, chain, ("vocoder", engine.tol["name"], B, T, log))


@pytest.mark.parametrize("tuning", ["F32_TRUNK", "NO_FUSED_WIDE", "NO_FUSED_STACKS", "DEBUG_POISON_ARENA"])
def test_vocoder_is_its_chain_under_tuning(voc_sd, tuning):
    """The 16-bit mode on the fp32 trunk, with the C = 256 stack as two launches per layer, with the C = 128 and C = 64 stacks so, and
    on a handle whose arena is re-poisoned before every plan run."""
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import MODEL_VOCODER
    eng = _engine(2, getattr(_lib, "TUNE_" + tuning), {MODEL_VOCODER: voc_sd})
    kinds = set()
    for B, T in VOC_SHAPES:
        whole, chain, wf, cf, log = _voc_case(eng, voc_sd, B, T)
        assert wf == cf == 0, (wf, cf)
        _same(whole, chain, ("vocoder", tuning, B, T, log))
        kinds.update(l[0] for l in log)
    want = {"F32_TRUNK": {"two", "wide", "fused"}, "NO_FUSED_WIDE": {"two", "fused"}, "NO_FUSED_STACKS": {"two", "wide"},
            "DEBUG_POISON_ARENA": {"two", "wide", "fused"}}[tuning]
    assert kinds - {"cond", "pre", "up"} == want, kinds
    eng.close()


def test_vocoder_alternate_table_is_its_chain(engine):
    """test_gpu_models.ALT_TABLES["half_width_base2"]: 256, 128, 64 and 32 channels, dilations 2^i -- the 32-channel stack in front of the
    tail has no activated form in the 16-bit mode (raw fp32 tensors, both convolutions with their own prologue)."""
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.engine import MODEL_VOCODER
    from test_gpu_models import ALT_TABLES
    t = ALT_TABLES["half_width_base2"]
    spec = type("Spec", (synth.VocoderSpec,), dict(t))
    n = len(spec.upsample_scales)
    sd = synth.make_vocoder_state_dict(11, spec)
    cfg = {"voc_channels": spec.channels, "voc_cond_channels": spec.cond_channels, "voc_cond_layers": spec.cond_layers, "voc_n_stages": n,
           "voc_scales": list(spec.upsample_scales) + [0] * (8 - n), "voc_depth": list(spec.resstack_depth) + [0] * (8 - n),
           "voc_dilation_base": spec.dilation_base}
    eng = _engine(engine.precision, 0, {MODEL_VOCODER: sd}, cfg)
    for B, T in VOC_SHAPES:
        whole, chain, wf, cf, log = _voc_case(eng, sd, B, T)
        assert wf & 3 == cf & 3 == 0, (wf, cf)
        _same(whole, chain, ("vocoder half_width_base2", engine.tol["name"], B, T, log))
        assert ("two_raw" in {l[0] for l in log}) == (engine.precision == 2), log
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the restore call as its stages
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unify", [False, True], ids=["plain", "unify_energy"])
def test_restore_gsr_is_its_stage_chain(engine, unify):
    """restore_gsr at 2 clips of 1.3 s: its log-mel is resunet_mel of the STFT's mel, its waveform op_from_log -> vocoder -> the peak
    (a maximum is exact) -> op_peak_trim, bit for bit."""
    from voicefixer_main_amd import synth
    wav = torch.from_numpy(synth.make_clips(2, 1.3, seed=88)[:, 0]).cuda()
    L = wav.shape[1]
    engine.take_flags()
    out, logmel = engine.restore_gsr(wav, unify_energy=unify, want_logmel=True)
    wf = engine.take_flags()
    mel = engine.op_stft(wav, want=("mel",))["mel"]
    lg = engine.resunet_mel(mel)
    _same(logmel, lg, ("restore_gsr logmel", engine.tol["name"], unify))
    den = engine.op_from_log(lg, mel, unify=unify)
    long = engine.vocoder(den)
    peak = long.abs().amax(dim=1)
    got = engine.op_peak_trim(long, L, peak.cpu())
    assert engine.take_flags() == wf
    _same(out, got, ("restore_gsr wav", engine.tol["name"], unify))


# ---------------------------------------------------------------------------------------------------------------------------------
# negative controls: the equalities above are not vacuous
# ---------------------------------------------------------------------------------------------------------------------------------
def test_control_swapped_skip_and_wrong_short_clip_differ(engine):
    from voicefixer_main_amd.engine import MODEL_UNET_MEL
    mel = _mel_input(3, 65, seed=65)      # Tpad 128: short_clip 1
    whole = engine.resunet_mel(mel)
    (swapped,) = PC.unet_chain(engine, MODEL_UNET_MEL, mel, [mel], swap_dec1=True, check_launches=False)
    _differ(whole, swapped, "dec1.1 on (skip, upsampled)")
    (wrong,) = PC.unet_chain(engine, MODEL_UNET_MEL, mel, [mel], short_clip=0)
    _differ(whole, wrong, "short_clip 0 at Tpad 128")
    engine.take_flags()


def test_control_wrong_slope_and_activated_tail_differ(engine, voc_sd):
    whole, chain, _, _, _ = _voc_case(engine, voc_sd, 2, 2, last_layer_slope=float(engine.cfg.voc_res_slope))
    _differ(whole, chain, "res_slope in front of an upsampler")
    whole, chain, _, _, _ = _voc_case(engine, voc_sd, 2, 2, tail_activated=True)
    _differ(whole, chain, "the tail on the activated tensor")
    engine.take_flags()
