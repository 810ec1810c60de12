"""GPU: the device noise mixers (Engine.mix_noise, csrc/mix.hip) and the list forms of simulate built on them -- the plain form bit
for bit the host function, the HQ forms inside a derived bound of the host function in float64, padding never read, every clip
independent of its batch -- and hard_clip_list."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import simulate  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
C = 4096           # kClipChunk (csrc/clip_batch.h): samples per workgroup, and per float64 partial sum of the level rule
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1, 3000]
F32 = np.float32
BAR = 16 * 2.0 ** -24      # the HQ forms against the float64 yardstick: see test_hq_forms_against_float64

LIST_FORMS = [simulate.add_noise_and_scale_list, simulate.add_noise_and_scale_with_HQ_list,
              simulate.add_noise_and_scale_with_HQ_with_Aug_list]
HOST_FORMS = [simulate.add_noise_and_scale, simulate.add_noise_and_scale_with_HQ, simulate.add_noise_and_scale_with_HQ_with_Aug]
NAMES = [("front", "noise"), ("hq", "front", "noise"), ("hq", "front", "aug", "noise")]      # the host functions' argument order


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


def _signals(nsig, lengths, seed):
    """nsig lists of float32 clips with the given lengths, each clip with a gain of its own"""
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(n) * rng.uniform(0.05, 1.5)).astype(F32) for n in lengths] for _ in range(nsig)]


def _assert_plain_equals_host(eng, front, noise, seed, **kw):
    """add_noise_and_scale_list of the items as ONE call == the loop over add_noise_and_scale with the same seed, bit for bit"""
    got = simulate.add_noise_and_scale_list(front, noise, rng=np.random.default_rng(seed), engine=eng, want_noisy=True, **kw)
    rng = np.random.default_rng(seed)
    for i, (f, n) in enumerate(zip(front, noise)):
        wf, wn, wsnr, wscale = simulate.add_noise_and_scale(f, n, rng=rng, **kw)
        gf, gn, gsnr, gscale, gnoisy = got[i]
        assert gf.dtype == gn.dtype == gnoisy.dtype == F32 and wf.dtype == F32
        assert np.array_equal(gf, wf) and np.array_equal(gn, wn), "item %d (%d samples)" % (i, len(f))
        assert gsnr == wsnr and gscale == wscale
        assert np.array_equal(gnoisy, wf + wn)
    return got


def test_plain_form_bit_for_bit(eng):
    front, noise = _signals(2, LENGTHS, seed=1)
    got = _assert_plain_equals_host(eng, front, noise, seed=11)
    assert all(-5 <= t[2] < 35 and 0.6 <= t[3] < 1.0 for t in got)


@pytest.mark.parametrize("snr", [30, -20])
def test_placement_of_the_peak(eng, snr):
    """the largest |sample| at index 0, at the last index, at an index that is no multiple of 4, negative -- in the front and in the
    noise.  snr = 30 dB: the noise ends 30 dB under the speech and the second peak comes from the speech / the mixture; snr = -20 dB:
    the noise ends 20 dB over it and the second peak comes from the noise / the mixture."""
    rng = np.random.default_rng(2)
    front, noise = [], []
    for n in (3000, C + 1):
        for where in ("front", "noise"):
            for pos, value in ((0, 0.9), (n - 1, 0.9), (1001, 0.9), (1001, -0.9)):
                f, z = (rng.uniform(-0.5, 0.5, n).astype(F32) for _ in range(2))
                (f if where == "front" else z)[pos] = value
                front.append(f)
                noise.append(z)
    got = _assert_plain_equals_host(eng, front, noise, seed=12, snr_l=snr, snr_h=snr)
    for f, z, (gf, gn, _, scale, gnoisy) in zip(front, noise, got):      # the case is what it claims to be
        peak = max(np.abs(gf).max(), np.abs(gn).max(), np.abs(gnoisy).max()) / F32(scale)
        assert abs(peak - 1) < 1e-6
        assert (np.abs(gn).max() > np.abs(gf).max()) == (snr < 0)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_padding_is_not_data(eng, form):
    """Engine.mix_noise on rows that hold 100 x the clip's peak past its length == on rows padded with zeros; the output rows are
    zero past the length.  The row stride is odd, so three rows of four start off a 16-byte boundary."""
    lengths = [3000, 1, 257, C + 1, 2999, 2 * C - 1]
    L = 2 * C + 3
    sig = _signals(len(NAMES[form]), lengths, seed=3 + form)
    clean = {k: np.zeros((len(lengths), L), F32) for k in NAMES[form]}
    for k, clips in zip(NAMES[form], sig):
        for b, c in enumerate(clips):
            clean[k][b, :len(c)] = c
    dirty = {k: v.copy() for k, v in clean.items()}
    for k in dirty:
        for b, n in enumerate(lengths):
            dirty[k][b, n:] = 100 * np.abs(clean[k][b]).max() * (-1) ** b
    kw = dict(lengths=lengths, noise_weight=[10 ** (s / 20) for s in (-3, 0, 5, 10, 20, 30)], scale=[0.6, 0.7, 0.8, 0.9, 0.95, 1.0],
              want_noisy=True)

    def run(x):
        return {k: v.cpu().numpy() for k, v in eng.mix_noise(**{k: torch.from_numpy(v).to(DEV) for k, v in x.items()}, **kw).items()}
    a, b = run(clean), run(dirty)
    assert set(a) == set(NAMES[form]) | {"noisy"}
    for k in a:
        assert a[k].shape == (len(lengths), L) and np.array_equal(a[k], b[k], equal_nan=True)
        for r, n in enumerate(lengths):
            assert np.isfinite(b[k][r, :n]).all() and b[k][r, :n].any() and not b[k][r, n:].any()


@pytest.mark.parametrize("form", [0, 1, 2])
def test_batch_invariance(eng, form):
    """each clip of a ragged batch (odd row stride) == its own single-clip call (a 1-D tensor), bit for bit"""
    lengths = [C + 1, 3000, 2 * C + 1, 65, 1]
    L = 2 * C + 1
    sig = _signals(len(NAMES[form]), lengths, seed=20 + form)
    weights, scales = [10 ** (s / 20) for s in (-5, 0, 7, 15, 34)], [0.6, 0.7, 0.8, 0.9, 1.0]
    batch = {}
    for k, clips in zip(NAMES[form], sig):
        x = np.zeros((len(lengths), L), F32)
        for b, c in enumerate(clips):
            x[b, :len(c)] = c
        batch[k] = torch.from_numpy(x).to(DEV)
    got = eng.mix_noise(**batch, lengths=lengths, noise_weight=weights, scale=scales, want_noisy=True)
    for b, n in enumerate(lengths):
        own = eng.mix_noise(**{k: torch.from_numpy(clips[b]).to(DEV) for k, clips in zip(NAMES[form], sig)},
                            noise_weight=weights[b], scale=scales[b], want_noisy=True)
        for k in got:
            assert own[k].shape == (n,) and torch.equal(got[k][b, :n], own[k]), "clip %d, %s" % (b, k)


def test_second_slice_of_a_call(eng):
    """130 clips in one call (128 clips travel per set of launches, kMixMaxClips) == rows 0-127 and rows 128-129 each in a call of
    their own, bit for bit: form 2 with the noisy output, a weight and a scale per clip"""
    B = 130
    lengths = [(1, 65, 257, C - 1, C, C + 1, 3000)[b % 7] for b in range(B)]
    L = C + 4
    rng = np.random.default_rng(80)
    batch = {}
    for k, clips in zip(NAMES[2], _signals(4, lengths, seed=81)):
        x = np.zeros((B, L), F32)
        for b, c in enumerate(clips):
            x[b, :len(c)] = c
        batch[k] = torch.from_numpy(x).to(DEV)
    weights, scales = [10 ** (s / 20) for s in rng.uniform(-5, 35, B)], list(rng.uniform(0.6, 1.0, B))

    def run(lo, hi):
        return eng.mix_noise(**{k: v[lo:hi] for k, v in batch.items()}, lengths=lengths[lo:hi], noise_weight=weights[lo:hi],
                             scale=scales[lo:hi], want_noisy=True)
    whole, head, tail = run(0, B), run(0, 128), run(128, B)
    assert set(whole) == set(NAMES[2]) | {"noisy"}
    for k in whole:
        assert whole[k].shape == (B, L) and torch.equal(whole[k], torch.cat([head[k], tail[k]])), k
        assert bool(torch.isfinite(whole[k]).all()) and all(bool(whole[k][b, :n].any()) for b, n in enumerate(lengths))


@pytest.mark.parametrize("form", [1, 2])
def test_hq_forms_against_float64(eng, form):
    """Forms 1 and 2 against the single-clip host function evaluated on float64 copies of the same float32 inputs with the same
    seeded draws: |device - yardstick| <= 16 * 2^-24 * |yardstick| per sample on every returned signal.  The longest path is the
    noise's: 5 elementwise float32 roundings (/ peak, / level ratio, / weight, * 1 / second peak, * scale), 4 scalars rounded to
    float32 (the level ratio, the weight, 1 / second peak, the scale), and a second peak taken from a float32 mixture whose samples
    carry up to 5 roundings: 14 half-ulps (2^-24 each) to first order, rounded up to 16.  (The device's float64 level sums and the
    yardstick's differ by ~1e-16: nothing at this scale.)  Two device calls on the same batch are bit-identical: the sums are
    deterministic."""
    sig = _signals(len(NAMES[form]), LENGTHS, seed=30 + form)
    got = LIST_FORMS[form](*sig, rng=np.random.default_rng(31), engine=eng, want_noisy=True)
    again = LIST_FORMS[form](*sig, rng=np.random.default_rng(31), engine=eng, want_noisy=True)
    rng = np.random.default_rng(31)
    nsig = len(NAMES[form])
    worst = 0.0
    for i in range(len(LENGTHS)):
        want = HOST_FORMS[form](*[s[i].astype(np.float64) for s in sig], rng=rng)
        assert got[i][nsig] == want[nsig] and got[i][nsig + 1] == want[nsig + 1]      # snr, scale: the same draws
        for k, g, w, g2 in zip(NAMES[form], got[i], want, again[i]):
            assert g.dtype == F32 and g.shape == w.shape
            err = np.abs(g.astype(np.float64) - w) / np.abs(w)
            worst = max(worst, err.max())
            assert (err <= BAR).all(), "item %d (%d samples), %s: %.2f * 2^-24" % (i, LENGTHS[i], k, err.max() * 2 ** 24)
            assert np.array_equal(g, g2)
        speech = got[i][NAMES[form].index("aug" if form == 2 else "front")]
        assert np.array_equal(got[i][-1], got[i][nsig - 1] + speech) and np.array_equal(got[i][-1], again[i][-1])
    print("form %d: worst error %.2f * 2^-24" % (form, worst * 2 ** 24))


def _with_HQ_f64(HQ, front, noise, w, scale, force_match):
    """add_noise_and_scale_with_HQ in float64 with a given weight, and the level rule as it is or forced on"""
    noise = noise / np.abs(noise).max()
    s = 1.0 / max(np.abs(HQ).max(), np.abs(front).max())
    HQ, front = HQ * s, front * s
    level = np.mean(np.abs(front))
    if level > 0.02 or force_match:
        noise = noise / (np.mean(np.abs(noise)) / level)
    noise = noise / w
    s = 1.0 / max(np.abs(noise + front).max(), np.abs(noise).max(), np.abs(front).max(), np.abs(HQ).max())
    return HQ * s * scale, front * s * scale, noise * s * scale


@pytest.mark.parametrize("form", [1, 2])
def test_both_sides_of_the_level_rule(eng, form):
    """item 0: the unified speech has mean |.| near 0.2, item 1 near 0.002 -- a factor of ten to either side of 0.02.  In item 1 the
    noise comes out unmatched: within the bar of the yardstick, far from what the matched rule would give."""
    n = C + 77
    rng = np.random.default_rng(40)
    speech = [rng.uniform(-0.4, 0.4, n).astype(F32), rng.uniform(-0.004, 0.004, n).astype(F32)]
    for s in speech:
        s[123] = 1.0      # the peak that unify_energy scales by
    others = [[(0.5 * s).astype(F32) for s in speech] for _ in range(form)]      # hq (and front in form 2): smaller peaks
    noise = [rng.standard_normal(n).astype(F32) for _ in speech]
    sig = others[:1] + ([speech] if form == 1 else [others[1], speech]) + [noise]      # the speech is front (1) / aug (2)
    for s, want_level in zip(speech, (0.2, 0.002)):
        assert 0.8 * want_level < np.abs(s).mean() < 1.2 * want_level
    got = LIST_FORMS[form](*sig, snr_l=10, snr_h=10, scale_lower=0.8, scale_upper=0.8, engine=eng)
    for i in range(2):
        want = HOST_FORMS[form](*[s[i].astype(np.float64) for s in sig], snr_l=10, snr_h=10, scale_lower=0.8, scale_upper=0.8)
        for k, g, w in zip(NAMES[form], got[i], want):
            assert (np.abs(g - w) <= BAR * np.abs(w)).all(), "item %d, %s" % (i, k)
    # the level rule in float64, as it is and forced on, with the speech as front (HQ plays no part in the noise's path here)
    for i, matched in ((0, True), (1, False)):
        args = (others[0][i].astype(np.float64), speech[i].astype(np.float64), noise[i].astype(np.float64), 10 ** (10 / 20), 0.8)
        as_is, forced = _with_HQ_f64(*args, force_match=False)[2], _with_HQ_f64(*args, force_match=True)[2]
        g = got[i][len(NAMES[form]) - 1]
        assert (np.abs(g - as_is) <= BAR * np.abs(as_is)).all()
        if matched:
            assert np.array_equal(as_is, forced)
        else:
            assert (np.abs(g - forced) > 1000 * BAR * np.abs(forced)).all()


def test_without_snr(eng):
    """snr_l = None: the weight step is skipped, snr is None, the plain form stays bit for bit the host function"""
    front, noise = _signals(2, [1, 257, C + 1, 3000], seed=50)
    got = _assert_plain_equals_host(eng, front, noise, seed=51, snr_l=None)
    assert all(t[2] is None for t in got)
    got = _assert_plain_equals_host(eng, front, noise, seed=51, snr_h=None)
    assert all(t[2] is None for t in got)


def test_silent_noise(eng):
    """an all-zero noise: 0 / 0 per sample, NaN everywhere -- what the host gives; no error, and the other clip of the batch is whole"""
    front, noise = _signals(2, [500, 700], seed=60)
    noise[0][:] = 0
    rng = np.random.default_rng(61)
    got = simulate.add_noise_and_scale_list(front, noise, rng=np.random.default_rng(61), engine=eng, want_noisy=True)
    for i in range(2):
        with np.errstate(all="ignore"):
            wf, wn, wsnr, wscale = simulate.add_noise_and_scale(front[i], noise[i], rng=rng)
        assert np.array_equal(got[i][0], wf, equal_nan=True) and np.array_equal(got[i][1], wn, equal_nan=True)
        assert got[i][2:4] == (wsnr, wscale)
    assert np.isnan(got[0][0]).all() and np.isnan(got[0][1]).all() and np.isnan(got[0][4]).all()
    assert np.isfinite(got[1][0]).all() and np.isfinite(got[1][1]).all()


def test_argument_errors_reach_python(eng):
    x = torch.ones((3, 500), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="clip 1 has 501 samples, the rows hold 500"):
        eng.mix_noise(x, x, lengths=[500, 501, 500])
    with pytest.raises(RuntimeError, match="clip 2 is empty"):
        eng.mix_noise(x, x, lengths=[500, 500, 0])
    with pytest.raises(RuntimeError, match="needs hq"):
        eng.mix_noise(x, x, aug=x)
    big = torch.ones((1025, 4), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="at most 1024"):
        eng.mix_noise(big, big)
    with pytest.raises(ValueError):
        eng.mix_noise(x, x[:, :499])
    ok = eng.mix_noise(x, x, hq=x, lengths=[500, 499, 1])      # and the handle still works
    assert set(ok) == {"front", "noise", "hq"} and bool(torch.isfinite(ok["hq"]).all())


def test_device_results_and_hard_clip(eng):
    """to_host=False: device tensors, the ones a to_host call returns; hard_clip_list on device float32 clips == hard_clip"""
    sig = _signals(4, [3000, 700], seed=70)
    host = simulate.add_noise_and_scale_with_HQ_with_Aug_list(*sig, rng=np.random.default_rng(71), engine=eng, want_noisy=True)
    dev = simulate.add_noise_and_scale_with_HQ_with_Aug_list(*[[torch.from_numpy(c).to(DEV) for c in s] for s in sig],
                                                             rng=np.random.default_rng(71), engine=eng, to_host=False, want_noisy=True)
    for h, d in zip(host, dev):
        assert len(d) == 7 and d[4:6] == h[4:6]
        for k in (0, 1, 2, 3, 6):
            assert isinstance(d[k], torch.Tensor) and d[k].device == DEV and d[k].dtype == torch.float32 and d[k].dim() == 1
            assert np.array_equal(d[k].cpu().numpy(), h[k])
    clips = [t[6] for t in dev]
    got = simulate.hard_clip_list(clips, 0.25, engine=eng, to_host=False)
    for g, c in zip(got, clips):
        want = simulate.hard_clip(c.cpu().numpy(), 0.25)
        assert isinstance(g, torch.Tensor) and g.device == DEV and np.array_equal(g.cpu().numpy(), want) and want.dtype == F32
    back = simulate.hard_clip_list(clips, 0.25, engine=eng)
    assert all(isinstance(b, np.ndarray) and np.array_equal(b, g.cpu().numpy()) for b, g in zip(back, got))
