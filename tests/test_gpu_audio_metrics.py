"""GPU: vfx_audio_metrics (score.hip) against the float64 restatement (tests/audio_metrics_f64.py), per-clip independence of the
batch, argument checks, and aggregate_score end to end behind handler_gsr_voicefixer."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import audio_metrics_f64 as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd.engine import Engine
    return Engine("cuda:0")


def _images(rng, B, T, F):
    t = (10.0 ** rng.normal(-1.0, 1.0, size=(B, T, F))).astype(np.float32)
    e = (t * (1.0 + 0.4 * rng.normal(size=t.shape))).clip(0, None).astype(np.float32)
    return e, t


@pytest.mark.parametrize("T,F,rows", [(7, 128, [7, 7]), (40, 1025, [40, 7, 33]), (75, 128, [75, 39]), (12, 7, [12, 9]),
                                      (70, 70, [70, 38, 71 - 1]), (9, 1025, [9])])
def test_ssim_kernel_vs_float64(eng, T, F, rows):
    rng = np.random.default_rng(T * 1000 + F)
    e, t = _images(rng, len(rows), T, F)
    got = eng.op_ssim(torch.from_numpy(e), torch.from_numpy(t), rows).cpu().numpy()
    want = [ref.ssim(e[b, :r].astype(np.float64), t[b, :r].astype(np.float64)) for b, r in enumerate(rows)]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    same = eng.op_ssim(torch.from_numpy(t), torch.from_numpy(t), rows).cpu().numpy()
    np.testing.assert_allclose(same, 1.0, rtol=0, atol=1e-12)


def test_sisdr_kernel_vs_float64(eng):
    rng = np.random.default_rng(11)
    lens = [50000, 16384, 16385, 3000, 70001]
    L = max(lens) + 7
    t = rng.normal(size=(len(lens), L)).astype(np.float32)
    e = (0.6 * t + rng.normal(size=t.shape) * np.array([0.01, 0.3, 1.0, 3.0, 0.02])[:, None]).astype(np.float32)
    got = eng.op_sisdr(torch.from_numpy(e), torch.from_numpy(t), lens).cpu().numpy()
    want = [ref.sisdr(e[b, :n], t[b, :n]) for b, n in enumerate(lens)]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def _pairs():
    from voicefixer_main_amd import simulate, synth
    out = []
    for i, (sec, mode) in enumerate(((0.5, "noise"), (1.1, "lowpass"), (0.8, "clip"), (1.6, "noise"))):
        n = int(sec * 44100) + 37 * i
        clean = (synth.speech_like(n, 300 + i) * 0.7).astype(np.float32)
        out.append((synth.degrade(clean, 300 + i, mode), clean))
    clean = (synth.speech_like(50000, 320) * 0.7).astype(np.float32)
    out.append((simulate.lowpass(clean, 4000, 44100, order=8, _type="cheby1").astype(np.float32), clean))
    out.append(((clean * 0.5 + 1e-3 * np.sin(np.arange(50000))).astype(np.float32), clean))
    # as read from PCM16 files: silence is exact zeros, not fp32 noise far below what an fp32 STFT resolves
    return [(_pcm(x), _pcm(y)) for x, y in out]


def _pcm(x):
    return ((np.asarray(x, np.float64) * 2 ** 15).astype(np.short) / 32768.0).astype(np.float32)


def _batch(pairs):
    lens = [len(t) for _, t in pairs]
    L = max(lens)
    e = np.zeros((len(pairs), L), np.float32)
    t = np.zeros((len(pairs), L), np.float32)
    for b, (x, y) in enumerate(pairs):
        e[b, :len(x)], t[b, :len(y)] = x, y
    return torch.from_numpy(e), torch.from_numpy(t), lens


def test_audio_metrics_vs_float64_pipeline(eng):
    pairs = _pairs()
    e, t, lens = _batch(pairs)
    got = eng.audio_metrics(e, t, lens).cpu().numpy()
    assert got.shape == (len(pairs), 9) and got.dtype == np.float64
    for b, (x, y) in enumerate(pairs):
        want = ref.audio_metrics(x, y)
        g = got[b]
        assert abs(g[0] - want[0]) < 1e-6, (b, g[0], want[0])
        for k in (1, 5):
            assert abs(g[k] - want[k]) < 1e-4 * abs(want[k]), (b, ref.KEYS[k], g[k], want[k])
        for k in (2, 3, 6, 7):
            assert abs(g[k] - want[k]) < 2e-3, (b, ref.KEYS[k], g[k], want[k])
        for k in (4, 8):
            assert abs(g[k] - want[k]) < 1e-5, (b, ref.KEYS[k], g[k], want[k])


def test_each_clip_of_a_varlen_batch_equals_its_own_call(eng):
    from voicefixer_main_amd import synth
    rng = np.random.default_rng(2025)
    lens = sorted(int(v) for v in rng.uniform(2 * 44100, 8 * 44100, size=24))
    base = synth.make_clips(4, 8.1, seed=77)[:, 0]
    clean = [synth.speech_like(n, 500 + i).astype(np.float32) * 0.6 for i, n in enumerate(lens[:4])]
    pairs = [(base[i % 4, :n].copy(), (0.5 * base[(i + 1) % 4, :n] + 0.3 * base[i % 4, :n]).astype(np.float32))
             for i, n in enumerate(lens)]
    pairs[:4] = [(base[i, :len(c)].copy(), c) for i, c in enumerate(clean)]
    e, t, lens = _batch(pairs)
    got = eng.audio_metrics(e, t, lens).cpu()
    assert torch.isfinite(got).all()
    for b, n in enumerate(lens):
        own = eng.audio_metrics(e[b:b + 1, :n], t[b:b + 1, :n]).cpu()
        assert torch.equal(own[0], got[b]), (b, own[0] - got[b])
    # the same clips in another order and batch (a longer Lmax than any of them)
    idx = list(range(len(lens)))[::-3]
    pad = torch.zeros(len(idx), e.shape[1] + 5000)
    e2, t2 = pad.clone(), pad.clone()
    e2[:, :e.shape[1]], t2[:, :e.shape[1]] = e[idx], t[idx]
    again = eng.audio_metrics(e2, t2, [lens[i] for i in idx]).cpu()
    assert torch.equal(again, got[idx])


def test_bad_lengths_are_refused(eng):
    x = torch.rand(2, 8000) - 0.5
    eng.audio_metrics(x, x, [2646, 8000])
    with pytest.raises(RuntimeError, match="2645 samples"):
        eng.audio_metrics(x, x, [2645, 8000])
    with pytest.raises(RuntimeError, match="Lmax"):
        eng.audio_metrics(x, x, [3000, 8001])
    with pytest.raises(ValueError):
        eng.audio_metrics(x, x[:, :7000])
    torch.cuda.synchronize()


def _voicefixer(engine):
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.models import VoiceFixer
    m = VoiceFixer(None, channels=2, type_target="vocals", engine=engine)
    sd = {"generator.analysis_module." + k: v for k, v in synth.make_resunet_state_dict(0).items()}
    sd.update({"vocoder.model." + k: v for k, v in synth.make_vocoder_state_dict(1).items()})
    m.load_state_dict(sd)
    return m.eval().to(torch.device("cuda:0"))


def test_aggregate_score_after_the_handler(tmp_path):
    """handler_gsr_voicefixer restores a small list (its per-file JSON written as the reference's inference() does), then
    aggregate_score: JSON, CSV and result.json hold exactly what AudioMetrics.evaluation gives per pair."""
    from voicefixer_main_amd import handlers, metrics, synth
    from voicefixer_main_amd.engine import Engine
    eng = Engine("cuda:0", config={"precision": 1})
    data = tmp_path / "data"
    data.mkdir()
    lines = []
    for i, sec in enumerate((0.7, 1.3, 2.2)):
        n = int(sec * 44100)
        clean = synth.speech_like(n, 700 + i) * 0.6
        handlers.save_wave(clean, str(data / ("clean%d.wav" % i)))
        handlers.save_wave(synth.degrade(clean, 700 + i), str(data / ("noisy%d.wav" % i)))
        lines.append("%s %s" % (data / ("noisy%d.wav" % i), data / ("clean%d.wav" % i)))
    (tmp_path / "set.lst").write_text("\n".join(lines) + "\n")
    save = tmp_path / "out"
    (save / "vctk_demo").mkdir(parents=True)
    saved = dict(handlers._state)
    try:
        handlers._state["model"] = _voicefixer(eng)
        for line in lines:
            src, tgt = line.split(" ")
            dst = str(save / "vctk_demo" / os.path.basename(src))
            part1 = handlers.handler_gsr_voicefixer(src, dst, tgt, ckpt=None, device=torch.device("cuda:0"), meta={"unify_energy": False})
            metrics.write_json(part1, dst[:-4] + ".json")
    finally:
        handlers._state.clear()
        handlers._state.update(saved)
    metas = {"vctk_demo": {"rate": 44100, "list": str(tmp_path / "set.lst")}}
    res = metrics.aggregate_score(str(save), ["vctk_demo"], metas=metas, engine=eng)["vctk_demo"]
    judge = metrics.AudioMetrics(44100, engine=eng)
    assert list(res) == ["clean0.wav", "clean1.wav", "clean2.wav"]
    for i, name in enumerate(res):
        est = str(save / "vctk_demo" / ("noisy%d.wav" % i))
        one = judge.evaluation(est, str(data / name))
        assert list(one) == list(metrics.METRIC_KEYS)
        js = json.loads(open(est[:-4] + ".json").read())
        assert {k: js[k] for k in one} == one and "mel-lsd" in js and js == res[name]
    with open(save / "vctk_demo" / "vctk_demo.csv") as f:
        table = list(csv.reader(f))
    assert [r[0] for r in table] == ["", "clean0.wav", "clean1.wav", "clean2.wav", "mean"]
    out = json.loads(open(save / "vctk_demo" / "result.json").read())
    for j, k in enumerate(table[0][1:]):
        assert out[k] == pytest.approx(np.mean([res[n][k] for n in res]), rel=1e-12, abs=1e-12)
        assert float(table[-1][j + 1]) == out[k]
    eng.close()


def test_scoring_leaves_a_following_restore_unchanged():
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_VOCODER
    eng = Engine("cuda:0", config={"precision": 1})
    eng.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
    eng.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
    wav = torch.from_numpy(synth.make_clips(2, 1.5, seed=5)[:, 0])
    before = eng.restore_gsr(wav).cpu()
    e, t, lens = _batch(_pairs())
    eng.audio_metrics(e, t, lens)
    after = eng.restore_gsr(wav).cpu()
    assert torch.equal(before, after)
    eng.close()
