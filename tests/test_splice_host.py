"""CPU: the host side of the splice -- the bindings of vfx_stft_splice and vfx_band_power against the header, the weight, band and gain
rules of voicefixer_main_amd.splice against their second statement in tests/splice_f64.py, the list layer against a recording stub
engine, the float64 restatement against the two-spectrum blend it equals by linearity, and the planted defects against the tolerance
tests/test_gpu_splice.py holds the kernel to.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import splice_f64 as ref
from voicefixer_main_amd import _lib, splice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,nargs", [("vfx_stft_splice", 11), ("vfx_band_power", 10)])
def test_signature_matches_the_header(name, nargs):
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)      # the HOST / device notes hold commas
    res, args = _lib.SIGNATURES[name]
    assert len(decl.split(",")) == len(args) == nargs
    src = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "api.cpp")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, src)
    assert "splice.hip" in open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("w", [0, 1, 8])
@pytest.mark.parametrize("c", [0, 1, 5, 1025, 1040])
def test_ramp_weights(c, w):
    a = splice.ramp_weights(c, w)
    assert a.dtype == np.float32 and a.shape == (1025,)
    k = np.arange(1025)
    assert (a[k <= c - w - 1] == 1.0).all() and (a[k >= c] == 0.0).all()      # exact endpoints
    mid = (k > c - w - 1) & (k < c)
    assert ((a[mid] > 0.0) & (a[mid] < 1.0)).all() and mid.sum() == max(0, min(c - 1, 1024) - max(c - w, 0) + 1)
    assert (np.diff(a) <= 0.0).all()                                           # monotone
    for i in k[mid]:
        assert a[i] == np.float32(c - i) / np.float32(w + 1)                   # one float32 division
    assert np.abs(a - ref.weights(c, w)).max() <= 2.0 ** -24
    if w == 0:      # the hard mask of vfx_stft_lowpass
        assert np.array_equal(a, (k < c).astype(np.float32))


def test_ramp_weights_refuses_negative_arguments():
    for c, w in ((-1, 0), (5, -1)):
        with pytest.raises(ValueError):
            splice.ramp_weights(c, w)


def test_match_band():
    assert splice.match_band(300, 8) == (228, 292) == ref.match_band(300, 8, 64)
    assert splice.match_band(300, 8, 0) == (292, 292)
    assert splice.match_band(46, 8, 64) == (5, 38)           # the first five bins never count
    assert splice.match_band(10, 8, 64) == (5, 5)            # nothing under the ramp: an empty band
    assert splice.match_band(1025, 0, 64) == (961, 1025)
    for c in (0, 1, 5, 13, 14, 77, 1025, 1040):
        for w in (0, 1, 8):
            for m in (0, 1, 64):
                lo, hi = splice.match_band(c, w, m)
                assert (lo, hi) == ref.match_band(c, w, m) and 5 <= lo <= hi and hi - lo <= m


def test_match_gain():
    n = 640
    assert splice.match_gain(4.0, 1.0, n) == 2.0 and splice.match_gain(1.0, 4.0, n) == 0.5
    g = splice.match_gain(2.0, 1.0, n)
    assert g == float(np.float32(np.sqrt(2.0))) and isinstance(g, float)
    # the clamp, both ways
    assert splice.match_gain(1e6, 1.0, n) == float(np.float32(10.0 ** (12.0 / 20.0)))
    assert splice.match_gain(1.0, 1e6, n) == float(np.float32(10.0 ** (-12.0 / 20.0)))
    assert splice.match_gain(100.0, 1.0, n, max_gain_db=6.0) == float(np.float32(10.0 ** (6.0 / 20.0)))
    # a silent band: the eps clamp alone gives 1e-8 per term
    assert splice.match_gain(1e-8 * n, 1.0, n) == 1.0 and splice.match_gain(1.0, 4e-8 * n, n) == 1.0
    assert splice.match_gain(4.1e-8 * n, 16.4e-8 * n, n) == 0.5
    # an empty band
    assert splice.match_gain(0.0, 0.0, 0) == 1.0 and splice.match_gain(3.0, 1.0, 0) == 1.0
    rng = np.random.default_rng(0)
    for p_in, p_out in rng.uniform(0.01, 100.0, (50, 2)):
        assert abs(splice.match_gain(p_in, p_out, n) - ref.match_gain(p_in, p_out, n, 12.0)) <= 2.0 ** -22 * 4.0


# ---------------------------------------------------------------------------------------------------------------------------------
# splice_list against a stub engine that records what it is handed
# ---------------------------------------------------------------------------------------------------------------------------------
class Stub:
    """band_power: p_in = 4, p_out = 1 for every pair (a gain of 2); stft_splice: x + g y"""
    device = torch.device("cpu")

    def __init__(self):
        self.power_calls, self.splice_calls = [], []

    def band_power(self, a, b, lo_bins, hi_bins, lengths=None):
        self.power_calls.append(dict(shape=tuple(a.shape), lo=list(lo_bins), hi=list(hi_bins), lengths=list(lengths)))
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
        p = torch.ones((a.shape[0], 2), dtype=torch.float64)
        p[:, 0] = 4.0
        return p

    def stft_splice(self, x, y, cut_bins, lengths=None, ramp=0, gains=None):
        self.splice_calls.append(dict(shape=tuple(x.shape), cuts=list(cut_bins), lengths=list(lengths), ramp=ramp, gains=list(gains)))
        assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape
        return x + torch.tensor(gains, dtype=torch.float32)[:, None] * y


def _pairs(lengths, seed=3):
    rng = np.random.default_rng(seed)
    return ([rng.uniform(-1, 1, n).astype(np.float32) for n in lengths], [rng.uniform(-1, 1, n).astype(np.float32) for n in lengths])


def test_splice_list_hands_over_sorted_batches_of_at_most_128():
    lengths = [1025 + (37 * i) % 131 for i in range(131)]
    assert len(set(lengths)) == 131 and lengths != sorted(lengths)
    lengths[7], lengths[90] = 1024, 300      # too short for the reflection: the restored clip, untouched
    xs, ys = _pairs(lengths)
    cuts = [300 + i for i in range(131)]
    cuts[11] = 0                             # nothing of the input to keep
    eng = Stub()
    outs, gains = splice.splice_list(xs, ys, cuts, engine=eng, to_host=True)
    run = sorted((i for i in range(131) if i not in (7, 90, 11)), key=lambda i: lengths[i])
    assert len(run) == 128
    assert [c["lengths"] for c in eng.splice_calls] == [[lengths[i] for i in run]] == [c["lengths"] for c in eng.power_calls]
    call = eng.splice_calls[0]
    assert call["shape"] == (128, lengths[run[-1]]) and call["cuts"] == [cuts[i] for i in run] and call["ramp"] == 8
    assert call["gains"] == [2.0] * 128
    assert eng.power_calls[0]["lo"] == [cuts[i] - 8 - 64 for i in run] and eng.power_calls[0]["hi"] == [cuts[i] - 8 for i in run]
    for i in range(131):
        assert isinstance(outs[i], np.ndarray) and outs[i].dtype == np.float32 and outs[i].shape == (lengths[i],)
        if i in (7, 90, 11):
            assert np.array_equal(outs[i], ys[i]) and gains[i] == 1.0
        else:
            assert np.array_equal(outs[i], xs[i] + np.float32(2.0) * ys[i]) and gains[i] == 2.0
    # one more long clip: a second call for the longest; device form; match = 0 makes no band_power call
    lengths = [1025 + i for i in range(130)][::-1]
    xs, ys = _pairs(lengths, 4)
    eng = Stub()
    outs, gains = splice.splice_list(xs, [torch.from_numpy(y) for y in ys], 77, ramp=3, match=0, engine=eng)
    assert [len(c["lengths"]) for c in eng.splice_calls] == [128, 2] and eng.splice_calls[1]["lengths"] == [1153, 1154]
    assert eng.splice_calls[1]["shape"] == (2, 1154) and eng.splice_calls[1]["cuts"] == [77, 77] and eng.splice_calls[1]["ramp"] == 3
    assert eng.power_calls == [] and gains == [1.0] * 130
    for o, x, y in zip(outs, xs, ys):
        assert isinstance(o, torch.Tensor) and np.array_equal(o.numpy(), x + y)


def test_splice_list_refuses_unequal_pairs():
    xs, ys = _pairs([2000, 1500])
    with pytest.raises(ValueError, match="clip 1"):
        splice.splice_list(xs, [ys[0], ys[1][:-1]], 100, engine=Stub())
    with pytest.raises(ValueError, match="2 inputs and 1 restored"):
        splice.splice_list(xs, ys[:1], 100, engine=Stub())
    with pytest.raises(ValueError, match="3 cut-off bins for 2 clips"):
        splice.splice_list(xs, ys, [1, 2, 3], engine=Stub())
    with pytest.raises(ValueError, match="cut-off bin -1"):
        splice.splice_list(xs, ys, [1, -1], engine=Stub())


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(21)
    return rng.uniform(-1, 1, 4410).astype(np.float32), rng.uniform(-1, 1, 4410).astype(np.float32)


def test_restatement_equals_the_two_spectrum_blend(pair):
    x, y = pair
    for c, w, g in ((64, 8, 0.7), (46, 0, 1.0), (1025, 8, 1.7), (0, 8, 0.5)):
        a, b = ref.splice(x, y, c, w, g), ref.blend(x, y, c, w, g)
        err = float(np.abs(a - b).max())
        print("c=%d w=%d g=%g: max |splice - blend| = %.3g" % (c, w, g, err))
        assert err < 1e-12
    # the anchors, in float64: y == x gives x, c = 0 gives g y
    assert np.abs(ref.splice(x, x, 64, 8) - x).max() < 1e-12
    assert np.array_equal(ref.splice(x, y, 0, 8, 0.5), 0.5 * y.astype(np.float64))


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_the_tolerance_sees_each_planted_defect(pair, defect):
    x, y = pair
    for c in (46, 64, 1025):
        good = ref.splice(x, y, c, 8, 0.7)
        bad = ref.splice(x, y, c, 8, 0.7, defect=defect, row_len=5000)
        excess = float((np.abs(bad - good) / ref.tolerance(x, y, 0.7, good)).max())
        print("%s, c=%d: max |bad - good| = %.3g = %.3g tolerances" % (defect, c, np.abs(bad - good).max(), excess))
        assert excess > 10.0, (defect, c, excess)
