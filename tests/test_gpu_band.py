"""GPU: the bandwidth detector on the device (csrc/band.hip: k_band_energy, k_band_cut) -- vfx_band_energy against the float64
restatement of load_wav_energy (tests/band_f64.py) bin by bin, the cut-off bin exactly, batch independence with == on the doubles, the
refusals, and the Python surface (Engine.band_energy / band_cutoff, simulate.band_cutoff_list, handlers.load_wav_energy,
VoiceFixer / SSR_UNet.restore_prefiltered_list).

The bound of the energy profile is band_f64.energy_bound: the float32 transform's 11 * 2^-24 * sum|x w| per bin and frame through
log10(. + 1), a float64 summation term on top.  The cut-off bin is a discrete decision: every clip compared exactly has a margin of at
least ten times the bound of the two numbers the decision compares (band_f64.checked asserts it); tests/test_band_host.py shows that
the defects a padded-batch kernel can have move the profile by 10 .. 10^4 bounds, or move the bin.

As measured on an MI355X: max |e - e64| over the 1025 bins is 8.5e-8 .. 1.7e-6 against bounds of 6.5e-6 .. 1.5e-4 (1 - 2 % of the
bound in each of the twelve cases), and every bin equals the restatement's."""
import ctypes
import wave

import numpy as np
import pytest
import torch

import band_f64 as ref

pytestmark = pytest.mark.gpu

L65 = ref.L65
BATCH = [1025, 4533, L65]            # one padded batch, in this row order: 3, 9 and 56 frames at hop 512
HOPS = (512, 441)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd.engine import Engine
    return Engine("cuda:0", config={"precision": 1})


@pytest.fixture(scope="module")
def clips():
    """{n: clip} of every length of this file, each with its decision margin asserted at both hops"""
    return {n: ref.clip_for(n, HOPS) for n in ref.LENGTHS}


@pytest.fixture(scope="module")
def singles(eng, clips):
    """{(n, hop): (energy (1025,) float64, bin)} of every clip's own B = 1 call, computed once"""
    out = {}
    for n, x in clips.items():
        for hop in HOPS:
            e, c = eng.band_energy(torch.from_numpy(x), hop=hop)
            out[(n, hop)] = (e[0].cpu().numpy(), int(c[0]))
    return out


def _pad(rows, width, fill=0.0):
    x = torch.full((len(rows), width), fill)
    for b, c in enumerate(rows):
        x[b, :len(c)] = torch.from_numpy(np.asarray(c))
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# single clips against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("n", ref.LENGTHS)
def test_single_clip_vs_float64(eng, clips, singles, n, hop):
    from voicefixer_main_amd import simulate
    x = clips[n]
    got, cut = singles[(n, hop)]
    want, bound = ref.profile(x, hop), ref.energy_bound(x, hop)
    err = float(np.abs(got - want).max())
    print("n=%d hop=%d frames=%d max|e - e64|=%.3e bound=%.3e bin=%d" % (n, hop, ref.frames(n, hop), err, bound, cut))
    assert got.dtype == np.float64 and got.shape == (1025,) and want.max() > 1.0
    assert err <= bound, (n, hop, err, bound, int(np.abs(got - want).argmax()))
    assert cut == ref.cut_bin(x, hop)
    # the bin is the decision over the device's own profile: the same chain of float64 additions on the host
    assert cut == ref.decide(got)[0]
    hz = eng.band_cutoff(torch.from_numpy(x), hop=hop)
    assert hz == [ref.hz(cut)]
    if hop == 512:
        assert hz == [simulate.band_cutoff(x)] == [ref.cutoff(x)]
        assert eng.band_cutoff(torch.from_numpy(x), sample_rate=16000) == [ref.cutoff(x, 16000)]


def test_threshold_and_exclusive_prefix_on_white_noise(eng):
    """White noise: every bin holds energy, so an inclusive prefix or a counted bin 1024 moves the bin -- checked against the decision
    over the device's own profile, which is exact (the clip's margin against the float32 transform is not wide enough for the
    restatement's own bin to be asserted, and it is not)."""
    x = np.random.default_rng(0).standard_normal(30000).astype(np.float32)
    e, c = eng.band_energy(torch.from_numpy(x))
    e = e[0].cpu().numpy()
    assert np.abs(e - ref.profile(x)).max() <= ref.energy_bound(x)
    i = ref.decide(e)[0]
    assert int(c[0]) == i and abs(i - 974) <= 1
    assert ref.decide(e, inclusive=True)[0] == i - 1 and ref.decide(e, count_top=True)[0] == i + 1
    for thr in (0.5, 1.0, 1e-9):
        _, c = eng.band_energy(torch.from_numpy(x), threshold=thr)
        assert int(c[0]) == ref.decide(e, thr)[0]
    assert ref.decide(e, 1.0)[0] == 1024 and ref.decide(e, 1e-9)[0] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# a clip's numbers do not depend on the batch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HOPS)
def test_padded_batch_equals_single_calls(eng, clips, singles, hop):
    rows = [clips[n] for n in BATCH]
    for fill in (7.0, float("nan")):
        for order in ([0, 1, 2], [2, 0, 1]):
            x = _pad([rows[j] for j in order], L65 + 300, fill)
            lens = [BATCH[j] for j in order]
            e, c = eng.band_energy(x, lengths=lens, hop=hop)
            e, c = e.cpu().numpy(), c.cpu().tolist()
            for r, j in enumerate(order):
                want_e, want_c = singles[(BATCH[j], hop)]
                assert np.array_equal(e[r], want_e) and c[r] == want_c, (fill, order, r)
            assert eng.band_cutoff(x, lengths=lens, hop=hop) == [ref.hz(v) for v in c]


def test_130_clips_cross_the_sub_batch(eng):
    rng = np.random.default_rng(3)
    lens = [int(v) for v in rng.integers(1025, 1324, size=130)]
    lens[0], lens[127], lens[128], lens[129] = 1323, 1025, 1322, 1323
    rows = [ref.make_clip(n, 500 + i) for i, n in enumerate(lens)]
    e, c = eng.band_energy(_pad(rows, 1400, float("nan")), lengths=lens)
    e, c = e.cpu().numpy(), c.cpu().tolist()
    for i in (0, 1, 63, 126, 127, 128, 129):
        e1, c1 = eng.band_energy(torch.from_numpy(rows[i]))
        assert np.array_equal(e[i], e1[0].cpu().numpy()) and c[i] == int(c1[0]), i
    assert np.isfinite(e).all() and (e >= 0).all() and min(c) > 0
    # simulate.band_cutoff_list: the caller's order, a clip of at most 1024 samples on the host
    from voicefixer_main_amd import simulate
    some = [rows[5], rows[128], np.zeros(1000, np.float32), torch.from_numpy(rows[127]).to(eng.device)]
    assert simulate.band_cutoff_list(some, engine=eng) == [ref.hz(c[5]), ref.hz(c[128]), 0, ref.hz(c[127])]


def test_silent_clip(eng):
    x = torch.zeros(2, 5000)
    x[1, :3000] = torch.from_numpy(ref.make_clip(3000, 1))
    e, c = eng.band_energy(x, lengths=[5000, 3000])
    assert not e[0].any() and int(c[0]) == 0 and e[1].max() > 1.0 and int(c[1]) > 0
    assert eng.band_cutoff(x[0]) == [0]


def test_band_limited_clip_cuts_below_its_band(eng):
    rng = np.random.default_rng(11)
    x = torch.from_numpy((0.01 * rng.standard_normal(L65)).astype(np.float32))
    low = eng.stft_lowpass(x, 300).cpu() + torch.from_numpy((1e-7 * rng.standard_normal(L65)).astype(np.float32))
    _, c = eng.band_energy(torch.stack([low, x]))
    c = c.cpu().tolist()
    print("band-limited at bin 300 cuts at %d, unfiltered at %d" % tuple(c))
    assert 200 < c[0] < 300 < c[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(eng):
    from voicefixer_main_amd.engine import _ptr
    B, L = 2, 3000
    x = torch.zeros(B, L, device=eng.device)
    e = torch.full((B, 1025), -7.0, device=eng.device, dtype=torch.float64)
    c = torch.full((B,), -7, device=eng.device, dtype=torch.int32)

    def call(wav=x, b=B, lmax=L, lens=(L, L), hop=512, thr=0.95, cut=c):
        lens = None if lens is None else (ctypes.c_int * len(lens))(*lens)
        return eng.lib.vfx_band_energy(eng.h, _ptr(wav), b, lmax, lens, hop, thr, _ptr(e), _ptr(cut), eng._stream())

    cases = [(dict(wav=None), "NULL"), (dict(cut=None), "NULL"), (dict(b=0), "B > 0"), (dict(lens=(L, 1024)), "clip 1 has 1024 samples"),
             (dict(lens=(L + 1, L)), "clip 0 has 3001 samples"), (dict(hop=0), "hop = 0"), (dict(hop=2049), "hop = 2049"),
             (dict(thr=0.0), "threshold = 0"), (dict(thr=1.5), "threshold = 1.5"), (dict(thr=float("nan")), "threshold")]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        assert text in eng.lib.vfx_last_error().decode(), (kw, eng.lib.vfx_last_error())
    torch.cuda.synchronize()
    assert bool((e == -7.0).all()) and bool((c == -7).all())
    # lengths = NULL: every clip has Lmax samples; hop 2048 and threshold 1 are inside the range
    assert call(lens=None, hop=2048, thr=1.0) == 0
    torch.cuda.synchronize()
    assert not e.any() and not c.any()
    with pytest.raises(RuntimeError, match="clip 0 has 1024 samples"):
        eng.band_energy(torch.zeros(1024))
    with pytest.raises(ValueError, match="3 lengths for 2 clips"):
        eng.band_energy(x, lengths=[L, L, L])


# ---------------------------------------------------------------------------------------------------------------------------------
# load_wav_energy and restore_prefiltered_list
# ---------------------------------------------------------------------------------------------------------------------------------
def test_load_wav_energy_reads_and_resamples(eng, clips, tmp_path):
    from voicefixer_main_amd import handlers
    x = clips[L65]
    pcm = np.round(x.astype(np.float64) * 32768.0).astype("<i2")
    for rate in (44100, 22050):
        path = str(tmp_path / ("clip%d.wav" % rate))
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(pcm.tobytes())
        wav, cutoff = handlers.load_wav_energy(path, 44100, engine=eng)
        want = handlers.load_wav(path, 44100)
        assert isinstance(wav, np.ndarray) and wav.dtype == np.float32 and np.array_equal(wav, want)
        assert cutoff == eng.band_cutoff(torch.from_numpy(want))[0] and 0 < cutoff < 22050
        if rate == 44100:
            assert cutoff == ref.cutoff(ref.checked(want))


@pytest.mark.parametrize("kind", ["voicefixer", "ssr_unet"])
def test_restore_prefiltered_list_is_restore_list_of_lowpass_each(clips, kind):
    from voicefixer_main_amd import models, simulate, synth
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_UNET_SPEC, MODEL_VOCODER
    e = Engine("cuda:0", config={"precision": 1})
    if kind == "voicefixer":
        e.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
        e.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
        model = models.VoiceFixer(engine=e)
    else:
        e.load_state_dict(MODEL_UNET_SPEC, synth.make_resunet_state_dict(2))
        model = models.SSR_UNet(engine=e)
    wavs = [torch.from_numpy(clips[4533]), torch.zeros(3000), torch.from_numpy(clips[L65]), torch.from_numpy(clips[2048])]
    out, cutoffs = model.restore_prefiltered_list(wavs)
    assert cutoffs == [ref.cutoff(clips[4533]), 0, ref.cutoff(clips[L65]), ref.cutoff(clips[2048])]
    keep = [0, 2, 3]
    low = simulate.lowpass_each([wavs[i] for i in keep], [cutoffs[i] for i in keep], 44100, 5, "stft", engine=e, to_host=False)
    filtered = list(wavs)
    for i, y in zip(keep, low):
        assert y.shape == wavs[i].shape and not torch.equal(y.cpu(), wavs[i])
        filtered[i] = y
    want = model.restore_list(filtered)
    assert len(out) == 4
    for i in range(4):
        assert out[i].shape == wavs[i].shape and torch.equal(out[i], want[i]), i
    e.close()
