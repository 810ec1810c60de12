"""GPU: the 16 kHz branch of the scores (vfx_audio_metrics_rate, stft_dft.hip) -- k_stft_dft per element against the float64
restatement (tests/audio_metrics16k_f64.py) under the summation bound, the nine scores at the bars of test_gpu_audio_metrics.py,
per-clip independence of the batch, refusals, the 44.1 kHz path left bit for bit as it was, and AudioMetrics end to end."""
import ctypes

import numpy as np
import pytest
import torch

import audio_metrics16k_f64 as ref16

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd.engine import Engine
    return Engine("cuda:0")


def _ratio(err, bound):
    """err / bound where the bound is not zero (a frame of exact zeros has S_t = 0 and want = 0: there err must be 0)."""
    return float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())


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


def test_stft_dft_kernel_vs_float64_per_element(eng):
    """|got - want| <= 2 (743 + 4) u S_t + 2 u |want| with S_t = sum_n |x_n w_n| of the frame: one rounding per addition, operand and
    table entry of each of the two sums, doubled for the magnitude of the two, plus the square root's own rounding.  The mel image:
    that bound through the filterbank plus (372 + 2) u of the projection."""
    from voicefixer_main_amd import synth
    lens = [961, 1120, 1121, 2000, 10240 + 371, 16000]
    clips = [_pcm(synth.speech_like(n, 800 + i) * 0.7) for i, n in enumerate(lens)]
    wav = np.zeros((len(lens), max(lens) + 13), np.float32)
    for b, x in enumerate(clips):
        wav[b, :len(x)] = x
        wav[b, len(x):] = 0.25          # what lies past a clip's end must not be read
    sp, mel = eng.op_score_spectrogram(torch.from_numpy(wav), lens, rate=16000)
    sp, mel = sp.cpu().numpy().astype(np.float64), mel.cpu().numpy().astype(np.float64)
    T = max(ref16.num_frames(n) for n in lens)
    assert sp.shape == (len(lens), T, 372) and mel.shape == (len(lens), T, 80)
    fb, w = ref16.filterbank(), ref16.window()
    worst_sp = worst_mel = 0.0
    for b, x in enumerate(clips):
        t = ref16.num_frames(len(x))
        want = ref16.spectrogram(x)
        S = (np.abs(ref16.frames(x)) * w).sum(-1)
        bound = 2 * (743 + 4) * U32 * S[:, None] + 2 * U32 * np.abs(want)
        err = np.abs(sp[b, :t] - want)
        worst_sp = max(worst_sp, _ratio(err, bound))
        assert (err <= bound).all(), (b, _ratio(err, bound))
        want_mel = want @ fb
        bound_mel = bound @ fb + (372 + 2) * U32 * want_mel
        err_mel = np.abs(mel[b, :t] - want_mel)
        worst_mel = max(worst_mel, _ratio(err_mel, bound_mel))
        assert (err_mel <= bound_mel).all(), (b, _ratio(err_mel, bound_mel))
        assert not sp[b, t:].any() and not mel[b, t:].any()       # rows at or past the clip's frames: exact zeros
    print("k_stft_dft: largest error / bound = %.3g (spectrogram), %.3g (mel)" % (worst_sp, worst_mel))


def _pairs():
    from voicefixer_main_amd import simulate, synth
    out = []
    for i, (sec, mode) in enumerate(((0.5, "noise"), (1.1, "lowpass"), (0.8, "clip"), (1.6, "noise"))):
        n = int(sec * 16000) + 37 * i
        clean = (synth.speech_like(n, 300 + i) * 0.7).astype(np.float32)
        out.append((synth.degrade(clean, 300 + i, mode), clean))
    clean = (synth.speech_like(16000, 320) * 0.7).astype(np.float32)
    out.append((simulate.lowpass(clean, 2000, 16000, order=8, _type="cheby1").astype(np.float32), clean))
    out.append(((clean * 0.5 + 1e-3 * np.sin(np.arange(16000))).astype(np.float32), clean))
    return [(_pcm(x), _pcm(y)) for x, y in out]


def test_audio_metrics_16k_vs_float64_pipeline(eng):
    pairs = _pairs()
    e, t, lens = _batch(pairs)
    got = eng.audio_metrics(e, t, lens, rate=16000).cpu().numpy()
    assert got.shape == (len(pairs), 9) and got.dtype == np.float64
    for b, (x, y) in enumerate(pairs):
        want = ref16.audio_metrics(x, y)
        g = got[b]
        print(b, ["%.3g" % abs(g[k] - want[k]) for k in range(9)])
        assert abs(g[0] - want[0]) < 1e-6, (b, g[0], want[0])
        for k in (1, 5):
            assert abs(g[k] - want[k]) < 1e-4 * abs(want[k]), (b, ref16.KEYS[k], g[k], want[k])
        for k in (2, 3, 6, 7):
            assert abs(g[k] - want[k]) < 2e-3, (b, ref16.KEYS[k], g[k], want[k])
        for k in (4, 8):
            assert abs(g[k] - want[k]) < 1e-5, (b, ref16.KEYS[k], g[k], want[k])


def test_each_16k_clip_of_a_varlen_batch_equals_its_own_call(eng):
    from voicefixer_main_amd import synth
    rng = np.random.default_rng(2026)
    lens = sorted([int(v) for v in rng.uniform(16000, 64000, size=9)] + [961, 160 * 150, 160 * 321])
    assert len(set(lens)) == 12
    pairs = []
    for i, n in enumerate(lens):
        clean = (synth.speech_like(n, 600 + i) * 0.6).astype(np.float32)
        pairs.append((synth.degrade(clean, 600 + i, ("noise", "lowpass", "clip")[i % 3]).astype(np.float32), clean))
    e, t, lens = _batch(pairs)
    got = eng.audio_metrics(e, t, lens, rate=16000).cpu()
    assert torch.isfinite(got).all()
    for b, n in enumerate(lens):
        own = eng.audio_metrics(e[b:b + 1, :n], t[b:b + 1, :n], rate=16000).cpu()
        assert torch.equal(own[0], got[b]), (b, own[0] - got[b])
    # the same clips in another order and batch (a longer Lmax than any of them)
    idx = list(range(len(lens)))[::-3] + [1, 0]
    pad = torch.zeros(len(idx), e.shape[1] + 5000)
    e2, t2 = pad.clone(), pad.clone()
    e2[:, :e.shape[1]], t2[:, :e.shape[1]] = e[idx], t[idx]
    again = eng.audio_metrics(e2, t2, [lens[i] for i in idx], rate=16000).cpu()
    assert torch.equal(again, got[idx])


def test_refusals_and_the_44k_path_unchanged(eng):
    from voicefixer_main_amd import _lib, synth
    x = torch.rand(2, 3000) - 0.5
    eng.audio_metrics(x, x, [961, 3000], rate=16000)
    with pytest.raises(RuntimeError, match="960 samples"):
        eng.audio_metrics(x, x, [960, 3000], rate=16000)
    with pytest.raises(RuntimeError, match="Lmax"):
        eng.audio_metrics(x, x, [2000, 3001], rate=16000)
    with pytest.raises(RuntimeError, match="44100 and 16000"):
        eng.audio_metrics(x, x, rate=22050)
    with pytest.raises(RuntimeError, match="44100 and 16000"):
        eng.op_score_spectrogram(x, rate=22050)
    # 44.1 kHz: vfx_audio_metrics and vfx_audio_metrics_rate(44100) are the same bits, before and after calls at 16 kHz
    pairs = []
    for i, n in enumerate((2646, 30000, 22050 + 441)):
        clean = _pcm(synth.speech_like(n, 900 + i) * 0.6)
        pairs.append((_pcm(synth.degrade(clean, 900 + i, "noise")), clean))
    e, t, lens = _batch(pairs)
    e, t = e.to(eng.device), t.to(eng.device)
    before = eng.audio_metrics(e, t, lens).cpu()
    assert torch.equal(before, eng.audio_metrics(e, t, lens, rate=44100).cpu())
    old = torch.empty((len(lens), 9), device=eng.device, dtype=torch.float64)
    _lib.check(eng.lib.vfx_audio_metrics(eng.h, ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(t.data_ptr()), len(lens), e.shape[1],
                                         (ctypes.c_int * len(lens))(*lens), ctypes.c_void_p(old.data_ptr()), eng._stream()),
               "vfx_audio_metrics")
    assert torch.equal(old.cpu(), before)
    e16, t16, lens16 = _batch(_pairs())
    eng.audio_metrics(e16, t16, lens16, rate=16000)
    assert torch.equal(eng.audio_metrics(e, t, lens).cpu(), before)
    torch.cuda.synchronize()


def test_audio_metrics_class_end_to_end_at_16k(eng, tmp_path):
    from voicefixer_main_amd import handlers, metrics, synth
    pairs, files = [], []
    for i, sec in enumerate((0.9, 2.3, 1.4)):
        n = int(sec * 16000) + 11 * i
        clean = synth.speech_like(n, 950 + i) * 0.6
        noisy = synth.degrade(clean.astype(np.float32), 950 + i, "noise")
        a, b = str(tmp_path / ("noisy%d.wav" % i)), str(tmp_path / ("clean%d.wav" % i))
        handlers.save_wave(noisy, a, sample_rate=16000)
        handlers.save_wave(clean, b, sample_rate=16000)
        files.append((a, b))
        pairs.append((handlers.load_wav(a, 16000), handlers.load_wav(b, 16000)))
    res = metrics.AudioMetrics(16000, engine=eng, stoi=True).evaluation_list(files)
    order = sorted(range(3), key=lambda i: len(pairs[i][1]))          # evaluation_list scores sorted by length
    e, t, lens = _batch([pairs[i] for i in order])
    scores = eng.audio_metrics(e, t, lens, rate=16000).cpu().numpy()
    st = eng.stoi(e, t, lens, fs=16000).cpu().numpy()
    for j, i in enumerate(order):
        assert isinstance(res[i], dict) and list(res[i]) == ["sisdr", "stoi"] + list(metrics.METRIC_KEYS[1:])
        assert res[i]["stoi"] == float(st[j])
        for k, key in enumerate(metrics.METRIC_KEYS):
            assert res[i][key] == float(scores[j, k]), (i, key)
