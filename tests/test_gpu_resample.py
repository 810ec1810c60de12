"""GPU: the device resampler (Engine.resample, csrc/resample.hip) against scipy.signal.resample_poly bit for bit, its window form,
the streamed reader of handlers.py and the model / handler surfaces that resample on the device."""
import wave
from math import gcd

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 48000, 88200, 96000)
PAIRS = [(r, 44100) for r in RATES] + [(44100, 8000), (44100, 16000), (44100, 48000)]
DEV = torch.device("cuda:0")


def _pair(sr_in, sr_out):
    g = gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def _scipy(x, sr_in, sr_out):
    return torch.from_numpy(resample_poly(x, *_pair(sr_in, sr_out)))


def _signals(rng, n):
    """a random signal and a full-scale one (every sample at -1 or at the largest PCM16 value)"""
    return (rng.uniform(-1, 1, n).astype(np.float32),
            np.where(rng.random(n) < 0.5, -1.0, 32767 / 32768).astype(np.float32))


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


@pytest.fixture(scope="module")
def models_eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_UNET_SPEC, MODEL_VOCODER
    e = Engine("cuda:0", config={"precision": 1})
    e.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
    e.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
    e.load_state_dict(MODEL_UNET_SPEC, synth.make_resunet_state_dict(2))
    return e


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_resample_equals_resample_poly(eng, sr_in, sr_out):
    """Every supported pair, lengths 1, 2, below hl / up, around one workgroup's run of outputs (256 R, R = 1, 2, 4), and 10 s."""
    up, down = _pair(sr_in, sr_out)
    hl = 10 * max(up, down)
    rng = np.random.default_rng(sr_in * 7 + sr_out)
    lengths = {1, 2, max(1, hl // up - 1), 10 * sr_in}
    for run in (256, 512, 1024, 2048):
        n = -(-run * down // up)        # the input length whose output length is about `run`
        lengths.update({n - 1, n, n + 1})
    for n in sorted(lengths):
        for x in _signals(rng, n):
            y, n_out = eng.resample(torch.from_numpy(x).to(DEV), sr_in, sr_out)
            want = _scipy(x, sr_in, sr_out)
            assert n_out == want.shape[0] and y.dtype == torch.float32
            assert torch.equal(y.cpu(), want), (sr_in, sr_out, n, (y.cpu() - want).abs().max())


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 44100), (16000, 44100), (44100, 8000)])
def test_resample_batch_with_lengths(eng, sr_in, sr_out):
    """16 clips of different lengths in one call: every row is its own single-clip call and scipy's, zero past its output length."""
    rng = np.random.default_rng(5)
    lengths = [1, 2, 17, 300, 1023, 4096, 9999] + [int(v) for v in rng.integers(1, 3 * sr_in, 9)]
    L = max(lengths)
    batch = torch.zeros((16, L), dtype=torch.float32)
    clips = []
    for i, n in enumerate(lengths):
        clips.append(rng.uniform(-1, 1, n).astype(np.float32))
        batch[i, :n] = torch.from_numpy(clips[-1])
    for i, n in enumerate(lengths):       # garbage past each clip's end must not leak into it
        batch[i, n:] = 7.0
    y, out_lengths = eng.resample(batch.to(DEV), sr_in, sr_out, lengths=lengths)
    y = y.cpu()
    for i, n in enumerate(lengths):
        want = _scipy(clips[i], sr_in, sr_out)
        assert out_lengths[i] == want.shape[0]
        assert torch.equal(y[i, :out_lengths[i]], want), i
        assert torch.equal(y[i, :out_lengths[i]], eng.resample(torch.from_numpy(clips[i]).to(DEV), sr_in, sr_out)[0].cpu()), i
        assert not y[i, out_lengths[i]:].any(), i
    # the same rate is resample_poly's copy
    same, same_lengths = eng.resample(batch.to(DEV), sr_in, sr_in, lengths=lengths)
    assert same_lengths == lengths
    for i, n in enumerate(lengths):
        assert torch.equal(same[i, :n].cpu(), torch.from_numpy(clips[i])) and not same[i, n:].any(), i


def test_resample_second_slice_of_a_call(eng):
    """66 clips of 50 .. 500 samples at 3/2 in one call (64 clips travel per launch, kResampleMaxClips), the rows padded with 7.0:
    every row is scipy's on that clip alone, zero past its output length"""
    sr_in, sr_out = 32000, 48000
    assert _pair(sr_in, sr_out) == (3, 2)
    rng = np.random.default_rng(21)
    B = 66
    lengths = [int(v) for v in rng.integers(50, 501, B)]
    lengths[63], lengths[64], lengths[65] = 500, 50, 499
    batch = torch.full((B, 503), 7.0, dtype=torch.float32)
    clips = [rng.uniform(-1, 1, n).astype(np.float32) for n in lengths]
    for i, c in enumerate(clips):
        batch[i, :len(c)] = torch.from_numpy(c)
    y, out_lengths = eng.resample(batch.to(DEV), sr_in, sr_out, lengths=lengths)
    y = y.cpu()
    assert y.shape == (B, 750)
    for i, c in enumerate(clips):
        want = _scipy(c, sr_in, sr_out)
        assert out_lengths[i] == want.shape[0] and torch.equal(y[i, :out_lengths[i]], want), i
        assert not y[i, out_lengths[i]:].any(), i


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 44100), (16000, 44100), (8000, 44100), (44100, 16000)])
def test_resample_windows_concatenate(eng, sr_in, sr_out):
    """Outputs over arbitrary [o0, o0 + n) windows, each from the minimal input window, concatenate to the whole result; a window
    that lacks one needed sample, at either end, is refused."""
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, 3 * sr_in + 123).astype(np.float32)
    whole = _scipy(x, sr_in, sr_out)
    n_out = whole.shape[0]
    cuts = sorted({0, n_out} | {int(v) for v in rng.integers(0, n_out, 9)} | {1, 2, 1025})
    parts = []
    for o0, o1 in zip(cuts[:-1], cuts[1:]):
        k0, k1 = eng.resample_window(x.shape[0], sr_in, sr_out, o0, o1 - o0)
        xw = torch.from_numpy(x[k0:k1]).to(DEV)
        y, _ = eng.resample(xw, sr_in, sr_out, lengths=[x.shape[0]], x0=k0, o0=o0, n_out=o1 - o0)
        parts.append(y.cpu())
        if o0 == cuts[len(cuts) // 2]:
            for a, b in ((k0 + 1, k1), (k0, k1 - 1)):
                if a > 0 or b < x.shape[0]:
                    with pytest.raises(RuntimeError, match="need input samples"):
                        eng.resample(torch.from_numpy(x[a:b]).to(DEV), sr_in, sr_out, lengths=[x.shape[0]], x0=a, o0=o0,
                                     n_out=o1 - o0)
    assert torch.equal(torch.cat(parts), whole)


def _write_pcm16(path, x, sr):
    """x (n, ch) float in [-1, 1] -> a PCM16 file"""
    with wave.open(path, "wb") as f:
        f.setnchannels(x.shape[1])
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((x * 32767).astype("<i2").tobytes())


def test_streaming_reader_resamples_on_device(eng, tmp_path):
    """_WavReader with an engine streams PCM16 files at other rates (nothing loaded in the constructor) and returns, concatenated,
    load_wav's values bit for bit -- mono and stereo at 48, 22.05 and 16 kHz, and a truncated 48 kHz file."""
    from voicefixer_main_amd import handlers
    rng = np.random.default_rng(13)
    cases = [(ch, sr) for sr in (48000, 22050, 16000) for ch in (1, 2)]
    for i, (ch, sr) in enumerate(cases):
        p = str(tmp_path / ("r%d.wav" % i))
        _write_pcm16(p, rng.uniform(-0.9, 0.9, (int(2.5 * sr) + i, ch)), sr)
        want = torch.from_numpy(handlers.load_wav(p, 44100))
        for seg in (44100, 3000, 10 ** 7):
            r = handlers._WavReader(p, 44100, engine=eng)
            assert r.whole is None and len(r) == want.shape[0], (ch, sr)
            parts = []
            while sum(a.shape[0] for a in parts) < len(r):
                parts.append(r.read_device(seg, DEV))
                assert parts[-1].shape[0] > 0
            r.close()
            assert torch.equal(torch.cat(parts).cpu(), want), (ch, sr, seg)
    # truncated data chunk: the header promises 3 s at 48 kHz, the file holds 1.7 s
    p = str(tmp_path / "t.wav")
    _write_pcm16(p, rng.uniform(-0.9, 0.9, (144000, 1)), 48000)
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:44 + 2 * 81600])
    want = torch.from_numpy(handlers.load_wav(p, 44100))
    r = handlers._WavReader(p, 44100, engine=eng)
    assert r.whole is None and len(r) == 132300
    parts = []
    while sum(a.shape[0] for a in parts) < len(r):
        parts.append(r.read_device(44100, DEV))
        if parts[-1].shape[0] == 0:
            break
    r.close()
    got = torch.cat(parts).cpu()
    assert len(r) == want.shape[0] and torch.equal(got, want)


def _run_handler(fn, src, dst, target, device_resample):
    from voicefixer_main_amd import handlers
    old = handlers.DEVICE_RESAMPLE
    handlers.DEVICE_RESAMPLE = device_resample
    try:
        return fn(src, dst, target, ckpt=None, device=DEV, needrefresh=False, meta={"unify_energy": False})
    finally:
        handlers.DEVICE_RESAMPLE = old


def test_handlers_device_resample_byte_identical(models_eng, tmp_path):
    """handler_gsr_voicefixer on a 70-s 48 kHz stereo file with a 48 kHz target (two segments), and handler_ssr_unet on a 16 kHz
    file: the device path writes the same bytes and returns the same metrics as the host path (DEVICE_RESAMPLE = False)."""
    from voicefixer_main_amd import handlers, synth
    from voicefixer_main_amd.models import SSR_UNet, VoiceFixer
    vf = VoiceFixer(None, channels=2, type_target="vocals", engine=models_eng)
    ssr = SSR_UNet(None, channels=1, engine=models_eng)
    rng = np.random.default_rng(17)
    for name, model, sr, ch in (("gsr", vf, 48000, 2), ("ssr", ssr, 16000, 1)):
        n = 70 * sr
        clip = synth.make_clips(1, n / 44100.0, seed=23)[0, 0][:n]
        x = np.stack([clip * (0.8 + 0.1 * c) for c in range(ch)], axis=1)
        src, tgt = str(tmp_path / (name + "_in.wav")), str(tmp_path / (name + "_tgt.wav"))
        _write_pcm16(src, np.clip(x, -1, 1), sr)
        _write_pcm16(tgt, np.clip(clip + 0.01 * rng.standard_normal(n), -1, 1)[:, None], sr)
        fn = handlers.handler_gsr_voicefixer if name == "gsr" else handlers.handler_ssr_unet
        handlers._state["model"] = model
        outs, mets = [], []
        for dev_rs in (False, True):
            dst = str(tmp_path / ("%s_out_%d.wav" % (name, dev_rs)))
            mets.append(_run_handler(fn, src, dst, tgt, dev_rs))
            outs.append(open(dst, "rb").read())
        assert outs[0] == outs[1], name
        assert mets[0] == mets[1] and set(mets[0]) == {"mel-lsd", "mel-sispec", "mel-non-log-sispec", "mel-ssim"}, (name, mets)


def test_models_take_other_rates(models_eng):
    """VoiceFixer.restore(x, sample_rate=16000) and SSR_UNet.restore_list([...], sample_rate=...) equal the same calls on
    scipy-resampled input; the default sample_rate leaves a call as it was."""
    from voicefixer_main_amd import synth
    from voicefixer_main_amd.models import SSR_UNet, VoiceFixer
    vf = VoiceFixer(None, channels=2, type_target="vocals", engine=models_eng)
    ssr = SSR_UNet(None, channels=1, engine=models_eng)
    x16 = synth.make_clips(2, 1.5, seed=29)[:, 0, :24000].copy()
    y = vf.restore(torch.from_numpy(x16).to(DEV), sample_rate=16000)
    want = vf.restore(torch.stack([_scipy(c, 16000, 44100) for c in x16]).to(DEV))
    assert y.shape == want.shape and torch.equal(y, want)
    assert torch.equal(vf.restore(torch.from_numpy(x16[:, None]).to(DEV), sample_rate=16000), want[:, None])
    for sr in (16000, 48000):
        clips = [synth.make_clips(1, s, seed=31 + i)[0, 0] for i, s in enumerate((0.7, 1.1, 0.9))]
        clips = [c[:int(len(c) * sr / 44100)] for c in clips]
        got = ssr.restore_list([torch.from_numpy(c) for c in clips], sample_rate=sr)
        ref = ssr.restore_list([_scipy(c, sr, 44100) for c in clips])
        assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, ref)), sr
        got = vf.restore_list([torch.from_numpy(c) for c in clips], sample_rate=sr)
        ref = vf.restore_list([_scipy(c, sr, 44100) for c in clips])
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), sr
