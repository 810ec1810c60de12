"""GPU tests of the bi_gru / dnn analysis modules (csrc/analysis.hip: k_dense, k_gru_seq) through every layer: vfx_analysis_mel,
vfx_select_analysis + vfx_restore_gsr(_varlen), models.VoiceFixer (forward, restore, restore_list, load_from_checkpoint) and
handlers.handler_gsr_voicefixer.  References: the reference's own module (tests/golden/gsr_analysis.npz) and the float64
restatement of tests/test_analysis_modules_host.py."""
import os

import numpy as np
import pytest
import torch

from conftest import TOL, _make_engine
from test_analysis_modules_host import MAKERS, reference_forward

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODULES = ["bi_gru", "dnn"]
SWITCHES = ("unet", "unet_small", "bi_gru", "dnn")


def _hp(module):
    return {"task": {"gsr": {"gsr_model": {"voicefixer": {s: s == module for s in SWITCHES}}}}, "model": {"mel_freq_bins": 128}}


def _mid(module):
    from voicefixer_main_amd.engine import MODEL_DNN_MEL, MODEL_GRU_MEL
    return MODEL_GRU_MEL if module == "bi_gru" else MODEL_DNN_MEL


@pytest.fixture(scope="module", params=[1, 0, 2], ids=["split-bf16", "fp32", "fp16-vocoder"])
def eng(request):
    """A handle with the synthetic mel ResUNet, vocoder, bi_gru and dnn weights."""
    e = _make_engine(request.param)
    for module in MODULES:
        e.load_state_dict(_mid(module), MAKERS[module]())
    return e


@pytest.fixture(scope="module")
def voc_sd_():
    from voicefixer_main_amd import synth
    return synth.make_vocoder_state_dict(1)


def _checkpoint_sd(module, voc_sd):
    sd = {"generator.analysis_module." + k: v for k, v in MAKERS[module]().items()}
    sd.update({"vocoder.model." + k: v for k, v in voc_sd.items()})
    return sd


def _voicefixer(eng, module, voc_sd):
    from voicefixer_main_amd.models import VoiceFixer
    m = VoiceFixer(_hp(module), channels=2, type_target="vocals", engine=eng)
    m.load_state_dict(_checkpoint_sd(module, voc_sd))
    assert m.analysis_module == module
    return m.eval().to(torch.device("cuda:0"))


def _mel(B, T, seed):
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-7.5, 1.5, size=(B, T, 128))).astype(np.float32)


def _close(got, ref, tol, what):
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert d.mean() < tol["logmel_l1"] and d.max() < tol["logmel_max"], (what, d.mean(), d.max())


@pytest.mark.parametrize("module", MODULES)
def test_forward_vs_reference_module_golden(eng, module, voc_sd_):
    g = np.load(os.path.join(G, "gsr_analysis.npz"))
    m = _voicefixer(eng, module, voc_sd_)
    try:
        for T in (37, 101):
            out = m(torch.from_numpy(g["mel_T%d" % T]).cuda())["mel"]
            assert out.shape == (2, 1, T, 128)
            _close(out.cpu().numpy(), g["%s_out_T%d_f64" % (module, T)], TOL[0], (module, T))
    finally:
        eng.select_analysis(0)


@pytest.mark.parametrize("module", MODULES)
def test_analysis_mel_vs_float64_restatement(eng, module):
    sd = MAKERS[module]()
    shapes = [(3, 1), (3, 2), (3, 37), (3, 1001)] + ([(1, 6001)] if module == "bi_gru" else [])
    for B, T in shapes:
        mel = _mel(B, T, seed=T)
        got = eng.analysis_mel(_mid(module), torch.from_numpy(mel)).cpu().numpy()
        _close(got, reference_forward(module, sd, mel), TOL[0], (module, B, T))
    assert eng.take_flags() == 0


@pytest.mark.parametrize("module", MODULES)
def test_analysis_mel_is_the_same_bytes_in_every_mode(module):
    """k_dense and k_gru_seq are fp32 FMA in every precision mode (analysis.hip's header): three handles, one result."""
    engines = [_make_engine(p) for p in (0, 1, 2)]
    for e in engines:
        e.load_state_dict(_mid(module), MAKERS[module]())
    for B, T in ((3, 37), (2, 101)):
        mel = torch.from_numpy(_mel(B, T, seed=T)).cuda()
        outs = [e.analysis_mel(_mid(module), mel) for e in engines]
        assert torch.isfinite(outs[0]).all()
        for p in (1, 2):
            assert torch.equal(outs[0], outs[p]), (module, B, T, p, (outs[0] - outs[p]).abs().max().item())
    for e in engines:
        assert e.take_flags() == 0
        e.close()


@pytest.mark.parametrize("module", MODULES)
def test_batch_is_bitwise_its_clips(eng, module):
    mel = torch.from_numpy(_mel(5, 123, seed=5)).cuda()
    batch = eng.analysis_mel(_mid(module), mel)
    for b in range(5):
        assert torch.equal(batch[b:b + 1], eng.analysis_mel(_mid(module), mel[b:b + 1])), b


@pytest.mark.parametrize("module", MODULES)
def test_frames_clips_are_their_own_calls(eng, module):
    frames = [90, 61, 7, 1]
    mel = torch.from_numpy(_mel(4, 90, seed=9)).cuda()
    mel[1, 61:] = -1.0          # padding rows are never read: no negative-input flag from them
    out = eng.analysis_mel(_mid(module), mel, frames=frames)
    for b, n in enumerate(frames):
        own = eng.analysis_mel(_mid(module), mel[b:b + 1, :n].contiguous())
        assert torch.equal(out[b:b + 1, :n], own), (b, n)
        assert (out[b, n:] == 0).all(), b
    assert eng.take_flags() == 0


@pytest.mark.parametrize("module", MODULES)
def test_negative_input_raises_the_to_log_flag(eng, module, voc_sd_):
    from voicefixer_main_amd import _lib
    mel = torch.from_numpy(_mel(2, 20, seed=3)).cuda()
    mel[1, 13, 127] = -1e-3
    eng.take_flags()
    eng.analysis_mel(_mid(module), mel)
    assert eng.take_flags() & _lib.FLAG_NEGATIVE_INPUT
    m = _voicefixer(eng, module, voc_sd_)
    try:
        with pytest.raises(AssertionError, match="negative"):
            m(mel[:, None])
    finally:
        eng.select_analysis(0)


@pytest.mark.parametrize("module", MODULES)
def test_restore_is_the_stage_chain_and_restore_list_its_clips(eng, module, voc_sd_):
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.models import from_log
    m = _voicefixer(eng, module, voc_sd_)
    try:
        wav = torch.from_numpy(synth.make_clips(2, 1.3, seed=21)[:, 0]).cuda()
        out, logmel = eng.restore_gsr(wav, want_logmel=True)
        mel = eng.stft(wav)["mel"]
        lg = eng.analysis_mel(_mid(module), mel)
        assert torch.equal(logmel, lg)
        voc = eng.vocoder(from_log(lg))
        L = wav.shape[-1]
        peak = voc.abs().amax(dim=1, keepdim=True)
        voc = torch.where(peak > 1.0, voc / peak, voc)
        off = (voc.shape[-1] - L) // 2
        chain = voc[:, off:off + L]
        d = (out - chain).abs().max().item()
        assert d < TOL[eng.precision]["voc_max"], d
        # restore (the model surface) is restore_gsr
        assert torch.equal(m.restore(wav[:, None])[:, 0], out)
        # mixed lengths: every clip the bytes of its own restore call
        lens = [30000, 52000, 44100, 71234, 30000]
        clips = [torch.from_numpy(synth.make_clips(1, n / 44100.0, seed=60 + i)[0, 0][:n]).cuda() for i, n in enumerate(lens)]
        res = m.restore_list(clips)
        for c, r in zip(clips, res):
            own = m.restore(c[None])[0]
            assert r.shape == c.shape and torch.equal(r, own)
    finally:
        eng.select_analysis(0)


def test_selecting_the_unet_again_is_the_default_path(eng):
    """Two fresh handles (the module fixture's front-end table was replaced by VoiceFixer's MelScale): one that ran both new
    modules and went back to the ResUNet, one that never had them -- the same bytes."""
    from voicefixer_main_amd import synth
    wav = torch.from_numpy(synth.make_clips(2, 1.1, seed=71)[:, 0]).cuda()
    lens = [wav.shape[-1], 30000]
    fresh, back = _make_engine(eng.precision), _make_engine(eng.precision)
    ref = fresh.restore_gsr(wav).clone()
    ref_vl = fresh.restore_gsr_varlen(wav, lens).clone()
    for module in MODULES:
        back.load_state_dict(_mid(module), MAKERS[module]())
        back.select_analysis(_mid(module))
        back.restore_gsr(wav)
        back.restore_gsr_varlen(wav, lens)
        back.select_analysis(0)
        assert torch.equal(back.restore_gsr(wav), ref), module
        assert torch.equal(back.restore_gsr_varlen(wav, lens), ref_vl), module
    with pytest.raises(RuntimeError, match="not an analysis module"):
        back.select_analysis(2)
    fresh.close()
    back.close()


def test_a_model_on_the_strict_twin_runs_the_selected_module():
    """The handlers re-run a saturated precision-2 file on VoiceFixer(hp, engine=engine.strict_twin()): that model has loaded no
    weights itself, so its forward must follow the module the twin handle selected -- not fall back to the ResUNet."""
    from voicefixer_main_amd.engine import MODEL_GRU_MEL
    from voicefixer_main_amd.models import VoiceFixer
    e = _make_engine(2)
    e.load_state_dict(MODEL_GRU_MEL, MAKERS["bi_gru"]())
    e.select_analysis(MODEL_GRU_MEL)
    twin = e.strict_twin()
    assert twin.precision == 1 and twin.analysis_model == MODEL_GRU_MEL
    m = VoiceFixer(_hp("bi_gru"), channels=2, type_target="vocals", engine=twin)
    assert m.analysis_module == "bi_gru"
    mel = torch.from_numpy(_mel(2, 50, seed=11)).cuda()
    assert torch.equal(m(mel[:, None])["mel"][:, 0], twin.analysis_mel(MODEL_GRU_MEL, mel))
    e.close()


def test_select_needs_finalized_weights():
    from voicefixer_main_amd.engine import Engine, MODEL_GRU_MEL
    e = Engine("cuda:0")
    with pytest.raises(RuntimeError, match="bi_gru.*not finalized"):
        e.select_analysis(MODEL_GRU_MEL)
    bad = MAKERS["bi_gru"]()
    bad["2.gru.weight_hh_l1"] = bad["2.gru.weight_hh_l1"][:, :128]
    with pytest.raises(RuntimeError, match="2.gru.weight_hh_l1"):
        e.load_state_dict(MODEL_GRU_MEL, bad)
    e.close()


def test_graph_capture_of_a_bi_gru_restore(eng):
    from voicefixer_main_amd import synth
    wav = torch.from_numpy(synth.make_clips(2, 1.0, seed=81)[:, 0]).cuda()
    eng.select_analysis(_mid("bi_gru"))
    try:
        eager = eng.restore_gsr(wav).clone()
        out = torch.empty_like(wav)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            eng.restore_gsr(wav, out=out)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                eng.restore_gsr(wav, out=out)
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(2):
            out.zero_()
            eng.replay(graph)
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
        del graph
        eng.unpin_plans()
    finally:
        eng.select_analysis(0)


def _handler_in_reference_order(model, src, dst):
    """eval_gsr_voicefixer.py:37-77 as written (a copy of test_gpu_surface.py's): per-segment calls with their host syncs."""
    from voicefixer_main_amd import handlers
    from voicefixer_main_amd.models import from_log, tensor2numpy
    dev = torch.device("cuda:0")
    wav_10k = handlers.load_wav(src, sample_rate=44100)
    res = []
    seg_length = 44100 * handlers.SEG_SECONDS
    break_point = seg_length
    while break_point < wav_10k.shape[0] + seg_length:
        segment = wav_10k[break_point - seg_length:break_point]
        _, mel_noisy, seg_t = handlers._pre(model, segment, dev)
        out_model = model(mel_noisy)
        denoised_mel = from_log(out_model["mel"])
        out = model.vocoder(denoised_mel)
        if torch.max(torch.abs(out)) > 1.0:
            out = out / torch.max(torch.abs(out))
        out, _ = handlers.trim_center(out, seg_t)
        res.append(out)
        break_point += seg_length
    out = torch.cat(res, -1)
    handlers.save_wave(tensor2numpy(out[0, ...]), fname=dst, sample_rate=44100)


def test_handler_with_a_bi_gru_checkpoint(tmp_path, voc_sd_):
    from voicefixer_main_amd import handlers, synth
    from voicefixer_main_amd.models import VoiceFixer
    ckpt = str(tmp_path / "bi_gru.ckpt")
    torch.save({"state_dict": _checkpoint_sd("bi_gru", voc_sd_), "hyper_parameters": {"hp": _hp("bi_gru")}}, ckpt)
    wav = synth.make_clips(1, 65.0, seed=91)
    src, a, b = str(tmp_path / "in.wav"), str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    handlers.save_wave(wav[0, 0], src)
    saved = dict(handlers._state)
    try:
        handlers._state["hp"] = _hp("bi_gru")
        handlers._state["model"] = None
        dev = torch.device("cuda:0")
        handlers.handler_gsr_voicefixer(src, a, None, ckpt=ckpt, device=dev, needrefresh=True, meta={"unify_energy": False})
        assert handlers._state["model"].analysis_module == "bi_gru"
        ref_model = VoiceFixer(_hp("bi_gru"), channels=2, type_target="vocals").load_from_checkpoint(ckpt).eval()
        _handler_in_reference_order(ref_model, src, b)
        assert open(a, "rb").read() == open(b, "rb").read()
        # a checkpoint whose saved hp names another module is refused, naming both
        with pytest.raises(ValueError, match="'dnn'.*'bi_gru'"):
            VoiceFixer(_hp("dnn"), channels=2, type_target="vocals").load_from_checkpoint(ckpt)
    finally:
        handlers._state.clear()
        handlers._state.update(saved)
