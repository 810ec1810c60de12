"""GPU: the splice of restored clips onto their inputs (Engine.stft_splice, k_stft_splice in csrc/stft.hip; Engine.band_power,
csrc/splice.hip; voicefixer_main_amd/splice.py; VoiceFixer / SSR_UNet.restore_spliced_list).

Every pair of a padded batch bit for bit what the chain of existing launches gives for it alone -- the product g y and the difference by
torch in float32, Engine.stft with phases, the two products and the ramp weights by torch, Engine.istft, the sum by torch -- in the
small-launch geometry (IH = 2) and the large one (IH = 16), zeros past a clip's length; the three exact anchors of the definition; rows
poisoned with NaN past their lengths; the float64 restatement (tests/splice_f64.py) within splice_f64.tolerance, which
tests/test_splice_host.py shows to see every planted defect; the band powers against float64 sums of Engine.stft's own magnitudes within
the float64 summation bound; the refusals of both entry points; the list layer and the two model methods.

As measured on an MI355X (test_against_float64, ramp 8, g = 0.7): max |got - ref| = 1.1e-07 (1765 samples, c = 46), 1.1e-07 (2500
samples, c = 64) and 4.3e-07 (4533 samples, c = 1025), against tolerances of 3.3e-05 .. 3.4e-05 at those samples; the band powers
equal the exactly rounded float64 sums of the squared magnitudes in 13 of 14 cases and differ by 1.2e-16 (relative) in the other."""
import ctypes
import math

import numpy as np
import pytest
import torch

import splice_f64 as ref
from voicefixer_main_amd import clips as _clips, splice

pytestmark = pytest.mark.gpu

HOP = 441
# the lengths and cuts of tests/test_gpu_stft_lowpass.py: 1025 the shortest clip the reflection allows; 1323 = 3 * 441; 1764 / 1765: an
# overlap-add group of 2 * 441 ends inside the clip and one sample later.  46: what 1000 Hz gives; 64: the lane boundary; 1024 / 1025
# straddle the bin lane 0 handles alone; 2000: everything is the input's
SMALL_LENGTHS = [1025, 1323, 1764, 1765, 2048, 2500, 4410 + 123]
SMALL_CUTS = [0, 1, 46, 64, 1024, 1025, 2000]
SMALL_GAINS = [1.0, 0.5, 1.7, 0.7, 1.0, 2.0, 0.3]


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


def _clip(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def _chain(eng, x, y, c, w, g):
    """One pair alone through the launches the kernel replaces -> (n,) float32 on the host"""
    n = x.shape[0]
    xt, yt = torch.from_numpy(x).to(eng.device), torch.from_numpy(y).to(eng.device)
    gy = yt * torch.tensor(np.float32(g), device=eng.device)                 # 1: one float32 product
    d = xt - gy                                                               # 2: one float32 subtraction
    a = torch.from_numpy(splice.ramp_weights(c, w)).to(eng.device)            # 3
    o = eng.stft(d[None], want_mel=False, want_sp=True, want_phase=True)      # 4
    re, im = o["sp"] * o["cos"], o["sp"] * o["sin"]
    zero, ramp = torch.zeros_like(re), (a > 0) & (a < 1)
    re = torch.where(a == 0, zero, torch.where(ramp, re * a, re))
    im = torch.where(a == 0, zero, torch.where(ramp, im * a, im))
    r = eng.istft(re, im, n)[0]                                               # 5
    return (gy + r).cpu().numpy()                                             # 6


@pytest.fixture(scope="module")
def small(eng):
    """The small batch: inputs, restored clips, and each pair's own chain result at ramps 0 and 8 (computed once, shared, never written)"""
    xs = [_clip(n, 100 + i) for i, n in enumerate(SMALL_LENGTHS)]
    ys = [_clip(n, 200 + i) for i, n in enumerate(SMALL_LENGTHS)]
    want = {w: [_chain(eng, x, y, c, w, g) for x, y, c, g in zip(xs, ys, SMALL_CUTS, SMALL_GAINS)] for w in (0, 8)}
    return xs, ys, want


def _pad(rows, width=None, fill=0.0):
    width = max(r.shape[0] for r in rows) if width is None else width
    x = torch.full((len(rows), width), fill)
    for b, r in enumerate(rows):
        x[b, :r.shape[0]] = torch.from_numpy(r)
    return x


def _run(eng, xs, ys, cuts, ramp, gains, fill=0.0, width=None):
    lengths = [c.shape[0] for c in xs]
    out = eng.stft_splice(_pad(xs, width, fill), _pad(ys, width, fill), cuts, lengths=lengths, ramp=ramp, gains=gains)
    assert out.dtype == torch.float32 and out.shape == (len(xs), width or max(lengths)) and out.device == eng.device
    return out.cpu().numpy()


def _assert_rows(out, want, lengths):
    for b, (w, n) in enumerate(zip(want, lengths)):
        assert w.dtype == np.float32 and w.shape == (n,)
        assert np.array_equal(out[b, :n], w), (b, n, float(np.abs(out[b, :n] - w).max()))
        assert not out[b, n:].any(), (b, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit the chain of existing launches, per pair alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ramp", [0, 8])
def test_small_batch_bit_identical_per_clip(eng, small, ramp):
    xs, ys, want = small
    assert len(xs) * eng.frames(max(SMALL_LENGTHS)) < 4096      # the launch with IH = 2
    out = _run(eng, xs, ys, SMALL_CUTS, ramp, SMALL_GAINS)
    _assert_rows(out, want[ramp], SMALL_LENGTHS)
    assert not np.array_equal(want[0][3], want[8][3])           # the ramp is not the hard mask
    assert eng.take_flags() == 0
    # a 1-D pair, scalar cut and gain
    one = eng.stft_splice(torch.from_numpy(xs[3]), torch.from_numpy(ys[3]), SMALL_CUTS[3], ramp=ramp, gains=SMALL_GAINS[3])
    assert one.shape == (SMALL_LENGTHS[3],) and np.array_equal(one.cpu().numpy(), want[ramp][3])


def test_large_batch_bit_identical_per_clip(eng):
    rng = np.random.default_rng(7)
    lengths = [int(v) for v in rng.integers(1025, 14201, size=128)]
    lengths[5] = max(lengths[5], 13671 + 17)
    edge = 16 * HOP - 1024      # the first sample the second overlap-add group of 16 hops owns
    lengths[40], lengths[41] = edge - 1, edge + 1
    cuts = [int(v) for v in rng.integers(0, 1101, size=128)]
    gains = [float(np.float32(v)) for v in rng.uniform(0.25, 4.0, size=128)]
    B, T = len(lengths), eng.frames(max(lengths))
    assert max(lengths) >= 13671 and T >= 32 and B * T >= 4096      # the launch with IH = 16
    xs = [_clip(n, 1000 + i) for i, n in enumerate(lengths)]
    ys = [_clip(n, 3000 + i) for i, n in enumerate(lengths)]
    out = _run(eng, xs, ys, cuts, 8, gains)
    _assert_rows(out, [_chain(eng, x, y, c, 8, g) for x, y, c, g in zip(xs, ys, cuts, gains)], lengths)
    assert eng.take_flags() == 0


def test_130_pairs_cross_the_sub_batch(eng):
    """More than 128 pairs run as consecutive sub-batches of both entry points: the rows on both sides of the cut are the single calls'"""
    rng = np.random.default_rng(3)
    lengths = [int(v) for v in rng.integers(1025, 1324, size=130)]
    lengths[0], lengths[127], lengths[128], lengths[129] = 1323, 1025, 1322, 1323
    cuts = [int(v) for v in rng.integers(20, 1025, size=130)]
    gains = [float(np.float32(v)) for v in rng.uniform(0.5, 2.0, size=130)]
    xs = [_clip(n, 5000 + i) for i, n in enumerate(lengths)]
    ys = [_clip(n, 6000 + i) for i, n in enumerate(lengths)]
    out = _run(eng, xs, ys, cuts, 8, gains, fill=float("nan"), width=1400)
    assert np.isfinite(out).all()
    bands = [splice.match_band(c, 8) for c in cuts]
    power = eng.band_power(_pad(xs, 1400, float("nan")), _pad(ys, 1400, float("nan")), [b[0] for b in bands], [b[1] for b in bands],
                           lengths=lengths).cpu().numpy()
    assert np.isfinite(power).all()
    for i in (0, 1, 63, 126, 127, 128, 129):
        xt, yt = torch.from_numpy(xs[i]), torch.from_numpy(ys[i])
        one = eng.stft_splice(xt, yt, cuts[i], ramp=8, gains=gains[i]).cpu().numpy()
        assert np.array_equal(out[i, :lengths[i]], one) and not out[i, lengths[i]:].any(), i
        assert np.array_equal(power[i], eng.band_power(xt, yt, *bands[i]).cpu().numpy()), i


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the exact anchors;  3. nothing at or past a clip's length is read
# ---------------------------------------------------------------------------------------------------------------------------------
def test_exact_anchors(eng, small):
    xs, ys, _ = small
    # y == x with g = 1 gives x, for any cut and ramp
    for ramp in (0, 8):
        out = _run(eng, xs, xs, SMALL_CUTS, ramp, None)
        _assert_rows(out, xs, SMALL_LENGTHS)
    # y == 0 with w = 0 gives the low-pass
    zeros = [np.zeros_like(x) for x in xs]
    low = eng.stft_lowpass(_pad(xs), SMALL_CUTS, lengths=SMALL_LENGTHS).cpu().numpy()
    out = _run(eng, xs, zeros, SMALL_CUTS, 0, None)
    assert np.array_equal(out, low) and low[1:].any()
    # c = 0 gives float32(g y)
    out = _run(eng, xs, ys, 0, 8, SMALL_GAINS)
    _assert_rows(out, [np.float32(g) * y for g, y in zip(SMALL_GAINS, ys)], SMALL_LENGTHS)


def test_rows_of_nan_past_the_lengths(eng, small):
    xs, ys, want = small
    out = _run(eng, xs, ys, SMALL_CUTS, 8, SMALL_GAINS, fill=float("nan"), width=max(SMALL_LENGTHS) + 700)
    _assert_rows(out, want[8], SMALL_LENGTHS)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_against_float64(eng, small):
    xs, ys, _ = small
    pick = [3, 5, 6]
    cuts, g = [46, 64, 1025], 0.7
    out = _run(eng, [xs[i] for i in pick], [ys[i] for i in pick], cuts, 8, g)
    for row, i, c in zip(out, pick, cuts):
        x, y = xs[i], ys[i]
        want = ref.splice(x, y, c, 8, g)
        err, tol = np.abs(row[:x.shape[0]] - want), ref.tolerance(x, y, g, want)
        j = int((err / tol).argmax())
        print("cut %d, %d samples: max |got - ref| = %.3g, worst sample %d: %.3g against a tolerance of %.3g"
              % (c, x.shape[0], err.max(), j, err[j], tol[j]))
        assert (err < tol).all(), (c, j, float(err[j]), float(tol[j]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. band_power
# ---------------------------------------------------------------------------------------------------------------------------------
BANDS = [(5, 38), (0, 1025), (64, 64), (1000, 1025), (63, 65), (228, 292), (1024, 1025)]


def test_band_power(eng, small):
    xs, ys, _ = small
    lo, hi = [b[0] for b in BANDS], [b[1] for b in BANDS]
    for fill in (0.0, float("nan")):
        got = eng.band_power(_pad(xs, None, fill), _pad(ys, None, fill), lo, hi, lengths=SMALL_LENGTHS)
        assert got.dtype == torch.float64 and got.shape == (7, 2) and got.device == eng.device
        got = got.cpu().numpy()
        for b, (x, y) in enumerate(zip(xs, ys)):
            one = eng.band_power(torch.from_numpy(x), torch.from_numpy(y), lo[b], hi[b])
            assert one.shape == (2,) and np.array_equal(one.cpu().numpy(), got[b]), (fill, b)      # a batch's rows are the single-clip calls
            if fill != 0.0:
                continue
            for col, sig in enumerate((x, y)):
                sp = eng.stft(torch.from_numpy(sig)[None], want_mel=False, want_sp=True)["sp"][0].cpu().numpy().astype(np.float64)
                terms = (sp[:, lo[b]:hi[b]] ** 2).ravel()      # the square of a float32 is exact in float64
                want, n = math.fsum(terms), terms.size
                assert n == (x.shape[0] // HOP + 1) * (hi[b] - lo[b])
                err = abs(got[b, col] - want)
                print("clip %d band [%d, %d) signal %d: %d terms, |got - want| / want = %.3g, bound %.3g"
                      % (b, lo[b], hi[b], col, n, err / want if want else 0.0, n * 2.0 ** -52))
                assert err <= n * 2.0 ** -52 * want, (b, col, err, want)
        assert not got[2].any() and got[[0, 1, 3, 4, 5, 6]].all()      # hi == lo: exact zeros
    # the restatement's powers, to the float32 transform's accuracy
    assert abs(got[5, 0] / ref.band_power(xs[5], 228, 292) - 1.0) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


def test_splice_refusals_launch_nothing(eng):
    from voicefixer_main_amd.engine import _ptr
    B, L = 2, 2048
    x = torch.zeros((B, L), device=eng.device)
    y = torch.zeros((B, L), device=eng.device)
    out = torch.full((B, L), 7.0, device=eng.device)

    def call(xx=x, yy=y, b=B, lens=(L, L), cuts=(10, 10), ramp=8, gains=(1.0, 1.0), dst=out):
        g = None if gains is None else (ctypes.c_float * len(gains))(*gains)
        return eng.lib.vfx_stft_splice(eng.h, _ptr(xx), _ptr(yy), b, L, _ints(lens), _ints(cuts), ramp, g, _ptr(dst), eng._stream())

    cases = [(dict(xx=None), "NULL"), (dict(yy=None), "NULL"), (dict(lens=None), "NULL"), (dict(cuts=None), "NULL"),
             (dict(dst=None), "NULL"), (dict(b=0), "B > 0"), (dict(b=-1), "B > 0"), (dict(lens=(L, 1024)), "clip 1 has 1024 samples"),
             (dict(lens=(L + 1, L)), "clip 0 has 2049 samples"), (dict(cuts=(10, -1)), "clip 1 has cut-off bin -1"),
             (dict(ramp=-1), "ramp = -1"), (dict(gains=(1.0, float("nan"))), "clip 1 has gain"),
             (dict(gains=(float("inf"), 1.0)), "clip 0 has gain"), (dict(dst=x), "out overlaps x"), (dict(dst=y), "out overlaps y"),
             (dict(xx=out), "out overlaps x")]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        assert text in eng.lib.vfx_last_error().decode(), (kw, eng.lib.vfx_last_error())
    with pytest.raises(RuntimeError, match="1024 samples"):
        eng.stft_splice(x[:, :1024], y[:, :1024], 10)
    with pytest.raises(ValueError, match="3 cut-off bins for 2 clips"):
        eng.stft_splice(x, y, [1, 2, 3])
    with pytest.raises(ValueError, match="must be equal"):
        eng.stft_splice(x, y[:, :-1], 10)
    torch.cuda.synchronize(eng.device)
    assert bool((out == 7.0).all())      # nothing ran
    assert call(gains=None) == 0 and not bool(out.any())      # the same buffers take a good call: the splice of silence


def test_band_power_refusals_launch_nothing(eng):
    from voicefixer_main_amd.engine import _ptr
    B, L = 2, 2048
    a = torch.zeros((B, L), device=eng.device)
    b = torch.zeros((B, L), device=eng.device)
    out = torch.full((B, 2), 7.0, device=eng.device, dtype=torch.float64)

    def call(aa=a, bb=b, n=B, lens=(L, L), lo=(5, 5), hi=(69, 69), dst=out):
        return eng.lib.vfx_band_power(eng.h, _ptr(aa), _ptr(bb), n, L, _ints(lens), _ints(lo), _ints(hi), _ptr(dst), eng._stream())

    cases = [(dict(aa=None), "NULL"), (dict(bb=None), "NULL"), (dict(lo=None), "NULL"), (dict(hi=None), "NULL"), (dict(dst=None), "NULL"),
             (dict(n=0), "B > 0"), (dict(lens=(L, 1024)), "clip 1 has 1024 samples"), (dict(lens=(L + 1, L)), "clip 0 has 2049 samples"),
             (dict(lo=(5, -1)), "clip 1 has the band [-1, 69)"), (dict(hi=(1026, 69)), "clip 0 has the band [5, 1026)"),
             (dict(lo=(5, 70)), "clip 1 has the band [70, 69)"), (dict(dst=a), "out overlaps a"), (dict(dst=b), "out overlaps b")]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        assert text in eng.lib.vfx_last_error().decode(), (kw, eng.lib.vfx_last_error())
    with pytest.raises(ValueError, match="3 lower bins for 2 clips"):
        eng.band_power(a, b, [1, 2, 3], 10)
    torch.cuda.synchronize(eng.device)
    assert bool((out == 7.0).all())      # nothing ran
    # the same buffers take a good call; lengths = NULL: every clip has L samples; silence: the eps clamp's 1e-8 per term
    assert call(lens=None, lo=(5, 7), hi=(69, 7)) == 0
    got = out.cpu().numpy()
    assert np.allclose(got[0], 1e-8 * 64 * (L // HOP + 1), rtol=1e-6, atol=0.0) and not got[1].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the list layer
# ---------------------------------------------------------------------------------------------------------------------------------
def _loop(eng, xs, ys, cuts, ramp, match, max_gain_db=12.0):
    outs, gains = [], []
    for x, y, c in zip(xs, ys, cuts):
        n, g = x.shape[0], 1.0
        if n <= 1024 or c == 0:
            outs.append(np.asarray(y))
            gains.append(g)
            continue
        xt, yt = torch.from_numpy(x), torch.from_numpy(y)
        if match:
            lo, hi = (min(k, 1025) for k in splice.match_band(c, ramp, match))
            p = eng.band_power(xt, yt, lo, hi).cpu().tolist()
            g = splice.match_gain(p[0], p[1], (n // HOP + 1) * (hi - lo), max_gain_db)
        outs.append(eng.stft_splice(xt, yt, c, ramp=ramp, gains=g).cpu().numpy())
        gains.append(g)
    return outs, gains


def test_splice_list_is_the_loop_over_single_clips(eng, small, monkeypatch):
    xs, ys, _ = small
    xs, ys = list(xs) + [_clip(1000, 7), _clip(3000, 8)], [0.5 * y for y in ys] + [_clip(1000, 9), 3.0 * _clip(3000, 10)]
    cuts = [300, 0, 46, 200, 1024, 1025, 2000, 100, 400]
    want, want_gains = _loop(eng, xs, ys, cuts, 8, 64)
    # (cut 0 and the short clip pass through; cut 2000 leaves no bin of the spectrum under the ramp)
    assert len(set(want_gains)) > 4 and want_gains[1] == want_gains[7] == want_gains[6] == 1.0 and want_gains[8] < 0.5 < want_gains[0]
    for to_host in (True, False):
        got, gains = splice.splice_list(xs, ys, cuts, engine=eng, to_host=to_host)
        assert gains == want_gains
        for g, w in zip(got, want):
            if not to_host:
                assert isinstance(g, torch.Tensor) and g.device == eng.device
                g = g.cpu().numpy()
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and np.array_equal(g, w)
    calls = []
    real = eng.band_power
    monkeypatch.setattr(eng, "band_power", lambda *a, **k: calls.append(1) or real(*a, **k))
    got, gains = splice.splice_list(xs, ys, cuts, match=0, engine=eng, to_host=True)
    assert calls == [] and gains == [1.0] * len(xs)
    for g, w in zip(got, _loop(eng, xs, ys, cuts, 8, 0)[0]):
        assert np.array_equal(g, w)
    splice.splice_list(xs, ys, cuts, engine=eng)
    assert calls == [1]      # one band_power call per batch
    assert eng.take_flags() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the model methods, with synthetic weights
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["voicefixer", "ssr_unet"])
def test_restore_spliced_list_is_splice_list_of_restore_list(kind):
    from voicefixer_main_amd import models, synth
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_UNET_SPEC, MODEL_VOCODER
    e = Engine("cuda:0", config={"precision": 1})
    if kind == "voicefixer":
        e.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
        e.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
        model = models.VoiceFixer(engine=e)
    else:
        e.load_state_dict(MODEL_UNET_SPEC, synth.make_resunet_state_dict(2))
        model = models.SSR_UNet(engine=e)
    # six band-limited clips of 1.0 .. 1.6 s: noise low-passed at a bin of its own, over a floor that keeps the detector's profile alive
    rng = np.random.default_rng(5)
    lengths = [44100, 48000, 52345, 57000, 61111, 70560]
    wavs = []
    for n, c in zip(lengths, (150, 200, 250, 300, 350, 400)):
        x = torch.from_numpy((0.05 * rng.standard_normal(n)).astype(np.float32))
        wavs.append(e.stft_lowpass(x, c).cpu() + torch.from_numpy((1e-7 * rng.standard_normal(n)).astype(np.float32)))
    restored = model.restore_list(wavs)
    bins = [int(e.band_energy(w)[1][0]) for w in wavs]      # the detector's bins, clip by clip
    assert all(100 < b < c for b, c in zip(bins, (150, 200, 250, 300, 350, 400))), bins
    want, want_gains = splice.splice_list(wavs, restored, bins, engine=e)
    out, info = model.restore_spliced_list(wavs)
    assert len(out) == len(info) == 6
    for i in range(6):
        assert out[i].shape == wavs[i].shape and torch.equal(out[i], want[i]), i
        assert not torch.equal(out[i], restored[i])
        assert info[i] == {"cut_bin": bins[i], "cutoff_hz": int(22050 * bins[i] / 1025), "gain": want_gains[i]}, i
    print("%s: bins %s gains %s" % (kind, bins, ["%.3f" % g for g in want_gains]))
    # a caller's bins are taken as given; the other parameters reach splice_list
    mine = [120, 0, 260, 90, 300, 77]
    want, want_gains = splice.splice_list(wavs, restored, mine, ramp=4, match=0, engine=e)
    out, info = model.restore_spliced_list(wavs, cut_bins=mine, ramp=4, match=0)
    for i in range(6):
        assert torch.equal(out[i], want[i]) and info[i] == {"cut_bin": mine[i], "cutoff_hz": int(22050 * mine[i] / 1025), "gain": 1.0}
    assert torch.equal(out[1], restored[1])
    with pytest.raises(ValueError, match="2 cut-off bins for 6 clips"):
        model.restore_spliced_list(wavs, cut_bins=[1, 2])
    # 16 kHz input is resampled first and comes back at 44.1 kHz lengths
    low = [torch.from_numpy((0.05 * rng.standard_normal(n)).astype(np.float32)) for n in (16000, 17001)]
    up = models._resample_list(e, low, 16000)
    assert [int(u.shape[0]) for u in up] == [44100, -(-17001 * 441 // 160)]
    out, info = model.restore_spliced_list(low, sample_rate=16000)
    out44, info44 = model.restore_spliced_list(up)
    for i in range(2):
        assert out[i].shape == up[i].shape and torch.equal(out[i], out44[i]) and info[i] == info44[i]
        assert 300 < info[i]["cut_bin"] < 420      # 8 kHz is bin 372
    e.close()
