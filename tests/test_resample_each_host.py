"""CPU: the per-clip resampler's host side -- the recurrence of k_resample_each (tests/resample_each_ref.py) against
scipy.signal.resample_poly, vfx_resample_each_out_len, and what simulate's "stft" list path and lowpass_collate_val hand an engine
(stand-in engines on the CPU that record their calls and answer with SciPy, the idea of tests/test_clip_batches_host.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import signal

import resample_each_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, simulate  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
PAIRS = [(7554, 1500), (2468, 2001), (22048, 700), (21998, 300)]      # (the other rate, clip length)


def _fs_down(c):
    return int(c / int(FS / 2) * FS)


# ------------------------------------------------------------------------------------------------------------ the recurrence
@pytest.mark.parametrize("rate,n", PAIRS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_poly_ref_is_resample_poly_bit_for_bit(rate, n, dtype):
    x = np.random.default_rng(rate).uniform(-1, 1, n).astype(dtype)
    for sr_in, sr_out in ((FS, rate), (rate, FS)):
        want = signal.resample_poly(x, sr_out, sr_in)
        got = ref.poly_ref(x, sr_out, sr_in)
        assert got.dtype == want.dtype == dtype and got.shape == want.shape
        assert np.array_equal(got, want), (sr_in, sr_out, np.abs(got - want).max())


def test_poly_ref_same_rate_is_a_copy():
    x = np.arange(5, dtype=np.float32)
    y = ref.poly_ref(x, 3, 3)
    assert np.array_equal(y, x) and y is not x


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_out_len():
    lib = _lib.load()
    for rate, _ in PAIRS:
        for sr_in, sr_out in ((FS, rate), (rate, FS)):
            up, down = Engine.resample_ratio(sr_in, sr_out)
            for n in (0, 1, 2, 1000):
                want = len(signal.resample_poly(np.zeros(n), up, down)) if n else 0
                assert lib.vfx_resample_each_out_len(n, sr_out, sr_in) == want == ref.out_len(n, up, down), (sr_in, sr_out, n)
    assert lib.vfx_resample_each_out_len(10, 0, 3) == -1 and lib.vfx_resample_each_out_len(10, 3, 0) == -1
    assert lib.vfx_resample_each_out_len(10, -1, 3) == -1 and lib.vfx_resample_each_out_len(-1, 1, 3) == -1
    assert lib.vfx_resample_each_out_len(10, 65537, 65536) == -1 and lib.vfx_resample_each_out_len(10, 65536, 65537) == -1
    assert lib.vfx_resample_each_out_len(10, 65536, 65535) == 11
    assert lib.vfx_resample_each_out_len(10, 2 * 65537, 2 * 65536) == -1      # the cap counts after the gcd
    assert lib.vfx_resample_each_out_len(10, 3 * 65536, 3 * 65535) == 11
    assert lib.vfx_resample_each_out_len(7, 200000, 100000) == 14
    # 44100 -> 44099 is taken here; the LDS kernel's predicate keeps its -1
    assert lib.vfx_resample_each_out_len(1000, 44099, 44100) == 1000 and lib.vfx_resample_out_len(1000, 44099, 44100) == -1
    assert Engine.resample_each_supported(44100, 44099) and not Engine.resample_supported(44100, 44099)
    assert Engine.resample_each_supported(44100, 29) and Engine.resample_each_supported(29, 44100)
    assert not Engine.resample_each_supported(65537, 65536) and not Engine.resample_each_supported(0, 44100)
    assert Engine.resample_each_out_len(1000, 44100, 44099) == 1000


def test_header_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert re.search(r"\bint64_t vfx_resample_each_out_len\(int64_t n_in, int up, int down\);", header)
    assert re.search(r"\bint vfx_resample_each\(vfx_handle\* h, const void\* x, int x_f64, int B,", header)
    assert len(_lib.SIGNATURES["vfx_resample_each"][1]) == 16
    assert "hipGraph capture" in header[header.index("vfx_resample with a rate pair per clip"):header.index("int vfx_resample_each(")]


# ------------------------------------------------------------------------------------------------------------ routing
class OldEngine:
    """An engine from before `resample_each`: `resample` alone."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def resample(self, x, sr_in, sr_out, lengths=None):
        up, down = Engine.resample_ratio(sr_in, sr_out)
        self.calls.append(dict(fn="resample", x=tuple(x.shape), dtype=x.dtype, rates=(sr_in, sr_out), lengths=list(lengths)))
        rows = [signal.resample_poly(x[b, :n].numpy(), up, down) for b, n in enumerate(lengths)]
        y = torch.zeros((len(rows), max(len(r) for r in rows)), dtype=torch.float32)
        for b, r in enumerate(rows):
            y[b, :len(r)] = torch.from_numpy(r.copy())
        return y, [len(r) for r in rows]

    sosfiltfilt_padlen = staticmethod(Engine.sosfiltfilt_padlen)

    def sosfiltfilt(self, x, sos, lengths=None):
        self.calls.append(dict(fn="sosfiltfilt", x=tuple(x.shape), dtype=x.dtype, lengths=list(lengths)))
        y = torch.zeros(x.shape, dtype=torch.float64)
        for b, n in enumerate(lengths):
            y[b, :n] = torch.from_numpy(signal.sosfiltfilt(sos, x[b, :n].numpy()).copy())
        return y


class EachEngine(OldEngine):
    """... and one with it: a rate pair per clip, SciPy's values, zeros past a row's output length."""

    def resample_each(self, x, sr_in, sr_out, lengths=None, n_out=None):
        B = x.shape[0]
        per_clip = lambda v: [int(v)] * B if np.ndim(v) == 0 else [int(r) for r in v]      # noqa: E731
        self.calls.append(dict(fn="resample_each", x=tuple(x.shape), dtype=x.dtype, sr_in=sr_in, sr_out=sr_out, lengths=list(lengths),
                               n_out=n_out))
        rows = [signal.resample_poly(x[b, :n].numpy(), *Engine.resample_ratio(i, o))
                for b, (n, i, o) in enumerate(zip(lengths, per_clip(sr_in), per_clip(sr_out)))]
        width = max(len(r) for r in rows) if n_out is None else n_out
        y = torch.zeros((B, width), dtype=x.dtype)
        for b, r in enumerate(rows):
            y[b, :min(len(r), width)] = torch.from_numpy(r[:width].copy())
        return y, [len(r) for r in rows]


LENGTHS = (902, 300, 2001, 301, 300, 0, 640)
CUTS = (1234, 3777, 1234, 11024, 15, 3777, 22050)
DTYPES = (np.float32, np.float32, np.float64, np.int16, np.float32, np.float32, np.float32)


def _seven():
    rng = np.random.default_rng(7)
    return [(rng.standard_normal(n) * 0.3).astype(d) if d != np.int16 else rng.integers(-3000, 3000, n).astype(d)
            for n, d in zip(LENGTHS, DTYPES)]


@pytest.fixture(scope="module")
def seven_want():
    """the single-clip results of the seven clips, computed once and left unchanged"""
    return [simulate.lowpass(c, h, FS, _type="stft") for c, h in zip(_seven(), CUTS)]


def test_stft_items_go_to_resample_each_by_dtype_and_length(monkeypatch, seven_want):
    monkeypatch.setattr(simulate, "MAX_BATCH", 2)
    clips = _seven()
    assert [_fs_down(c) for c in CUTS] == [2468, 7554, 2468, 22048, 29, 7554, 44100]
    eng = EachEngine()
    got = simulate.lowpass_each(clips, CUTS, FS, types="stft", engine=eng)
    low = lambda n, c: ref.out_len(n, _fs_down(c), FS)      # noqa: E731
    f32, f64 = torch.float32, torch.float64
    # float32: clips 1, 4 (300 samples), then 0 (902); float64: clip 2.  int16 (3), empty (5) and fs_down == fs (6): the host
    assert eng.calls == [
        dict(fn="resample_each", x=(2, 300), dtype=f32, sr_in=FS, sr_out=[7554, 29], lengths=[300, 300], n_out=None),
        dict(fn="resample_each", x=(2, low(300, 3777)), dtype=f32, sr_in=[7554, 29], sr_out=FS, lengths=[low(300, 3777), low(300, 15)], n_out=300),
        dict(fn="resample_each", x=(1, 902), dtype=f32, sr_in=FS, sr_out=[2468], lengths=[902], n_out=None),
        dict(fn="resample_each", x=(1, low(902, 1234)), dtype=f32, sr_in=[2468], sr_out=FS, lengths=[low(902, 1234)], n_out=902),
        dict(fn="resample_each", x=(1, 2001), dtype=f64, sr_in=FS, sr_out=[2468], lengths=[2001], n_out=None),
        dict(fn="resample_each", x=(1, low(2001, 1234)), dtype=f64, sr_in=[2468], sr_out=FS, lengths=[low(2001, 1234)], n_out=2001),
    ]
    for i, (g, w) in enumerate(zip(got, seven_want)):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == (LENGTHS[i],) and np.array_equal(g, w), i
    assert [w.dtype for w in seven_want[:3]] == [np.float32, np.float32, np.float64]
    dev = simulate.lowpass_each(clips, CUTS, FS, types="stft", engine=EachEngine(), to_host=False)
    for i, (d, w) in enumerate(zip(dev, seven_want)):
        assert isinstance(d, torch.Tensor) and d.device == eng.device and np.array_equal(d.numpy(), w) and d.numpy().dtype == w.dtype, i
    # lowpass_list: one cut-off for the list, the same path
    eng = EachEngine()
    got = simulate.lowpass_list(clips[:3], 3777, FS, _type="stft", engine=eng)
    assert [c["sr_out"] for c in eng.calls[::2]] == [[7554, 7554], [7554]] and [c["dtype"] for c in eng.calls[::2]] == [f32, f64]
    for c, g in zip(clips, got):
        assert np.array_equal(g, simulate.lowpass(c, 3777, FS, _type="stft"))


def test_a_pair_past_the_cap_takes_the_host():
    """No cut-off at 44.1 kHz is past the cap (M <= 44100); the list function's own fs_ori = 200 003 (a prime) with ratio 0.4 gives
    fs_down = 80 001, nothing to reduce -- past 65 536: the host function."""
    fs, ratio = 200003, 0.4
    assert not Engine.resample_each_supported(fs, int(ratio * fs))
    x = (np.random.default_rng(1).standard_normal(40) * 0.3).astype(np.float32)
    eng = EachEngine()
    got = simulate._stft_list([x], [ratio], eng, True, fs_ori=fs)
    assert eng.calls == [] and np.array_equal(got[0], simulate.stft_hard_lowpass(x, ratio, fs_ori=fs))


def test_engines_without_resample_each_keep_their_calls(monkeypatch, seven_want):
    """Per distinct cut-off, float32 clips at the pairs Engine.resample takes: 1000 Hz (44100 <-> 2000) and 4000 Hz (<-> 8000) do,
    none of the seven clips' cut-offs does."""
    monkeypatch.setattr(simulate, "MAX_BATCH", 2)
    eng = OldEngine()
    got = simulate.lowpass_each(_seven(), CUTS, FS, types="stft", engine=eng)
    assert not any(Engine.resample_supported(FS, _fs_down(c)) for c in CUTS[:6]) and eng.calls == []
    for g, w in zip(got, seven_want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    rng = np.random.default_rng(3)
    clips = [(rng.standard_normal(n) * 0.3).astype(d) for n, d in ((902, np.float32), (300, np.float32), (640, np.float32), (500, np.float64))]
    cuts = (1000, 1000, 4000, 1000)
    got = simulate.lowpass_each(clips, cuts, FS, types="stft", engine=eng)
    f32 = torch.float32
    assert eng.calls == [
        dict(fn="resample", x=(2, 902), dtype=f32, rates=(FS, 2000), lengths=[300, 902]),
        dict(fn="resample", x=(2, 41), dtype=f32, rates=(2000, FS), lengths=[14, 41]),
        dict(fn="resample", x=(1, 640), dtype=f32, rates=(FS, 8000), lengths=[640]),
        dict(fn="resample", x=(1, 117), dtype=f32, rates=(8000, FS), lengths=[117]),
    ]
    for c, h, g in zip(clips, cuts, got):
        w = simulate.lowpass(c, h, FS, _type="stft")
        assert g.dtype == w.dtype and np.array_equal(g, w)


# ------------------------------------------------------------------------------------------------------------ lowpass_collate_val
def test_lowpass_collate_val():
    L = 400
    rng = np.random.default_rng(5)
    batch = [{"fname": "item%d" % i, "vocals": (rng.standard_normal((L, 2)) * 0.3).astype(np.float32),
              "noise": (rng.standard_normal((L, 1)) * 0.3).astype(np.float32)} for i in range(3)]
    eng = EachEngine()
    got = simulate.lowpass_collate_val(batch, engine=eng)
    cuts = [1000, 2000, 4000, 8000, 12000]
    assert set(got) == ({"fname", "vocals", "noise"} | {k + "LR_%d" % c for k in ("vocals", "noise") for c in cuts}
                        | {"%s_%d" % (w, c) for w in ("cutoffs", "orders", "filters") for c in cuts})
    assert got["fname"] == ["item0", "item1", "item2"]
    for key in ("vocals", "noise"):
        assert got[key].shape == (3, L, 1) and got[key].dtype == torch.float32
        assert all(np.array_equal(got[key][i, :, 0].numpy(), batch[i][key][:, 0]) for i in range(3))
        for c in cuts:
            lr = got[key + "LR_%d" % c]
            assert lr.shape == (3, L, 1) and lr.dtype == torch.float32 and lr.device == eng.device
            for i in range(3):
                y = simulate.lowpass(batch[i][key][..., 0], highcut=c, fs=44100, order=8, _type="butter")
                y = simulate.lowpass(y, highcut=c, fs=44100, order=8, _type="stft")
                assert y.dtype == np.float64 and np.array_equal(lr[i, :, 0].numpy(), y.astype(np.float32)), (key, c, i)
    for c in cuts:
        assert got["cutoffs_%d" % c] == cuts and got["orders_%d" % c] == [] and got["filters_%d" % c] == []
    # the "stft" pass took the Butterworth pass's float64 rows as they were: no host function, one call pair per cut-off and key
    each = [c for c in eng.calls if c["fn"] == "resample_each"]
    assert len(each) == 2 * 2 * len(cuts) and all(c["dtype"] == torch.float64 and c["x"][0] == 3 for c in each)
    host = simulate.lowpass_collate_val(batch, engine=EachEngine(), to_host=True)
    assert all(torch.equal(host[k], got[k]) for k in got if isinstance(got[k], torch.Tensor))
