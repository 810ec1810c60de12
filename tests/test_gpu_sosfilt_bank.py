"""GPU: the zero-phase IIR filter with a design per clip (Engine.sosfiltfilt_bank, k_sosfilt_bank in csrc/sosfilt.hip) against
scipy.signal.sosfiltfilt with the clip's own design, and the per-clip forms of the degradation simulator built on it
(simulate.lowpass_each / bandpass_each / lowpass_collate).  Every comparison is exact."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FS = 44100
NYQ = FS / 2
DEV = torch.device("cuda:0")
TILE = 64          # kSosTile (csrc/vfx_internal.h)
MAX_CLIPS = 128    # kSosMaxClips: clips per launch pair
BLOCK_CLIPS = 4    # kSosBankBlockClips (csrc/sosfilt.hip): a block takes up to four clips of ONE section count
IIR = ("butter", "cheby1", "ellip", "bessel")


def _lowpass_sos(name, order, highcut):
    from voicefixer_main_amd import simulate
    return simulate._design(order, highcut / NYQ, "low", name, "lowpass")


# the low-pass designs of orders 2 .. 10 for the four IIR types (S = 1 .. 5, padlen 9 .. 33), then an order-5 and an order-10
# band-pass (S = 5 and 10, padlen 33 and 63)
BANK = [_lowpass_sos(name, order, 750 + 1700 * order + 300 * k) for k, name in enumerate(IIR) for order in range(2, 11)]
BANK += [signal.butter(5, [300 / NYQ, 3400 / NYQ], btype="band", output="sos"),
         signal.cheby1(10, 0.1, [300 / NYQ, 3400 / NYQ], btype="band", output="sos")]


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


def _edge_lengths(padlen, S):
    """padlen + 1, padlen + 2, one sample either side of and at the tile length and twice it, and the extended clip -- and the
    skewed cascade's S - 1 extra steps -- ending one sample either side of and at a tile edge: 26 kinds."""
    out = [padlen + 1, padlen + 2]
    for edge in (TILE, 2 * TILE):
        out += [edge - 1, edge, edge + 1]
    for tiles in (2, 3, 4):
        for d in (-1, 0, 1):
            out += [tiles * TILE - 2 * padlen + d, tiles * TILE - 2 * padlen - (S - 1) + d]
    return out


def _batch(clips, dtype, fill=7.0):
    lengths = [len(c) for c in clips]
    x = torch.full((len(clips), max(lengths) + 5), fill, dtype=dtype)
    for i, c in enumerate(clips):
        x[i, :len(c)] = torch.from_numpy(c).to(dtype)
    return x.to(DEV), lengths


@pytest.fixture(scope="module")
def mixed(eng):
    """37 clips of pairwise different lengths, each length one of the edge kinds of the clip's OWN design; a shuffled index
    assignment that uses some designs several times and some not at all.  SciPy's results per dtype, computed once."""
    rng = np.random.default_rng(37)
    index = [len(BANK) - 1, len(BANK) - 2] + [int(v) for v in rng.integers(0, len(BANK), 35)]
    index = [index[i] for i in rng.permutation(37)]
    assert len(set(index)) < 37 and len(set(index)) < len(BANK) and {len(BANK) - 1, len(BANK) - 2} <= set(index)
    lengths = []
    for i, f in enumerate(index):
        padlen, S = eng.sosfiltfilt_padlen(BANK[f]), BANK[f].shape[0]
        kinds = _edge_lengths(padlen, S)
        n = next(kinds[(i + k) % len(kinds)] for k in range(len(kinds)) if kinds[(i + k) % len(kinds)] > padlen
                 and kinds[(i + k) % len(kinds)] not in lengths)
        lengths.append(n)
    assert len(set(lengths)) == 37 and len({BANK[f].shape[0] for f in index}) >= 6
    clips = [rng.uniform(-1, 1, n) for n in lengths]
    want = {dtype: [signal.sosfiltfilt(BANK[f], c.astype(dtype)) for c, f in zip(clips, index)] for dtype in (np.float32, np.float64)}
    return {"index": index, "lengths": lengths, "clips": clips, "want": want}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mixed_sections_in_one_call(eng, mixed, dtype):
    """S = 1 .. 5 and 10 and padlen 9 .. 63 in ONE call, the rows padded with 7.0 past their end: every row is SciPy on that clip
    with its own design, its own single-design call, and zero past its length."""
    clips = [c.astype(dtype) for c in mixed["clips"]]
    x, lengths = _batch(clips, torch.from_numpy(clips[0]).dtype)
    y = eng.sosfiltfilt_bank(x, BANK, filter_index=mixed["index"], lengths=lengths)
    assert y.dtype == torch.float64 and y.shape == x.shape
    y = y.cpu()
    for i, (n, f) in enumerate(zip(lengths, mixed["index"])):
        assert torch.equal(y[i, :n], torch.from_numpy(mixed["want"][dtype][i].copy())), (i, n, f)
        assert torch.equal(y[i, :n], eng.sosfiltfilt(torch.from_numpy(clips[i]).to(DEV), BANK[f]).cpu()), (i, n, f)
        assert not y[i, n:].any(), (i, n, f)


@pytest.mark.parametrize("sos", [signal.cheby1(8, 0.1, 1000 / NYQ, output="sos"),
                                 signal.cheby1(10, 0.1, [300 / NYQ, 3400 / NYQ], btype="band", output="sos")], ids=["cheby1_8", "bp_cheby1_10"])
def test_uniform_bank_equals_the_single_design_path(eng, sos):
    padlen = eng.sosfiltfilt_padlen(sos)
    rng = np.random.default_rng(5)
    lengths = [padlen + 1, padlen + 2, 3000] + [int(v) for v in rng.permutation(np.arange(padlen + 3, 2999))[:16]]
    x, lengths = _batch([rng.uniform(-1, 1, n).astype(np.float32) for n in lengths], torch.float32)
    want = eng.sosfiltfilt(x, sos, lengths=lengths)
    assert torch.equal(eng.sosfiltfilt_bank(x, [sos], filter_index=[0] * len(lengths), lengths=lengths), want)
    # ... and the default index: clip b takes design b
    assert torch.equal(eng.sosfiltfilt_bank(x, [sos] * len(lengths), lengths=lengths), want)


def test_a_row_does_not_depend_on_its_company(eng, mixed):
    """The rows and their indices permuted together give the same rows; so does every clip alone (B = 1, and 1-D input)."""
    clips = [c.astype(np.float32) for c in mixed["clips"]]
    want = mixed["want"][np.float32]
    perm = [int(v) for v in np.random.default_rng(9).permutation(37)]
    x, lengths = _batch([clips[p] for p in perm], torch.float32)
    y = eng.sosfiltfilt_bank(x, BANK, filter_index=[mixed["index"][p] for p in perm], lengths=lengths).cpu()
    for j, p in enumerate(perm):
        assert torch.equal(y[j, :lengths[j]], torch.from_numpy(want[p].copy())), (j, p)
    for i, f in enumerate(mixed["index"]):
        y = eng.sosfiltfilt_bank(torch.from_numpy(clips[i]).to(DEV), BANK, filter_index=[f])
        assert y.shape == (len(clips[i]),) and torch.equal(y.cpu(), torch.from_numpy(want[i].copy())), i


def _check(eng, clips, bank, index):
    x, lengths = _batch(clips, torch.from_numpy(clips[0]).dtype)
    y = eng.sosfiltfilt_bank(x, bank, filter_index=index, lengths=lengths).cpu()
    for i, (c, f) in enumerate(zip(clips, index)):
        want = signal.sosfiltfilt(bank[f], c)
        assert np.isfinite(want).all(), (i, f)
        assert torch.equal(y[i, :len(c)], torch.from_numpy(want.copy())), (i, len(c), f)
        assert not y[i, len(c):].any(), (i, f)


def test_edge_sizes(eng):
    rng = np.random.default_rng(21)
    # groups whose clip counts are 1, 2 and 3 more than a multiple of the clips per block (S = 1, 3 and 5), interleaved
    designs = [_lowpass_sos("butter", 2, 3000), _lowpass_sos("ellip", 6, 5000), _lowpass_sos("cheby1", 10, 7000)]
    index = [0] * (8 * BLOCK_CLIPS + 1) + [1] * (5 * BLOCK_CLIPS + 2) + [2] * (3 * BLOCK_CLIPS + 3)
    index = [index[i] for i in rng.permutation(len(index))]
    _check(eng, [rng.uniform(-1, 1, int(n)).astype(np.float32) for n in rng.integers(40, 600, len(index))], designs, index)
    # exactly one clip per section count, S = 1 .. 16 (band-passes of orders 6 .. 16 give S = 6 .. 16)
    designs = [_lowpass_sos("butter", o, 4000) for o in (2, 4, 6, 8, 10)]
    designs += [signal.butter(o, [2000 / NYQ, 9000 / NYQ], btype="band", output="sos") for o in range(6, 17)]
    assert [d.shape[0] for d in designs] == list(range(1, 17))
    index = [int(v) for v in rng.permutation(16)]
    _check(eng, [rng.uniform(-1, 1, int(n)) for n in rng.integers(150, 900, 16)], designs, index)
    # 131 clips of 100 .. 400 samples, S = 1 .. 5 and 10 mixed: more than one launch pair takes
    index = [int(v) for v in rng.integers(0, len(BANK), MAX_CLIPS + 3)]
    _check(eng, [rng.uniform(-1, 1, int(n)).astype(np.float32) for n in rng.integers(100, 401, len(index))], BANK, index)


def test_three_second_segments(eng):
    """What the collator filters: 3 s float32 segments, one per order 2 .. 10, in one call."""
    rng = np.random.default_rng(3)
    designs = [_lowpass_sos(IIR[o % 4], o, 700 * o) for o in range(2, 11)]
    _check(eng, [rng.uniform(-1, 1, 3 * FS).astype(np.float32) for _ in designs], designs, list(range(9)))


def test_errors_launch_nothing(eng):
    from voicefixer_main_amd import _lib
    designs = [_lowpass_sos("butter", o, 4000) for o in (2, 3, 4, 10)]
    assert [eng.sosfiltfilt_padlen(d) for d in designs] == [9, 12, 15, 33]
    batch = torch.zeros((4, 500), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="greater than padlen, which is 33"):
        eng.sosfiltfilt_bank(batch, designs, filter_index=[0, 3, 1, 2], lengths=[500, 20, 20, 20])
    eng.sosfiltfilt_bank(batch, designs, filter_index=[3, 0, 1, 2], lengths=[500, 20, 20, 20])
    with pytest.raises(ValueError, match="each must be in"):
        eng.sosfiltfilt_bank(batch, designs, filter_index=[0, 4, 1, 2])
    with pytest.raises(ValueError, match="no filter_index"):
        eng.sosfiltfilt_bank(batch, designs[:3])
    with pytest.raises(ValueError, match="17 sections"):
        eng.sosfiltfilt_bank(batch, designs[:3] + [np.tile(designs[0], (17, 1))], filter_index=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="all ones"):
        eng.sosfiltfilt_bank(batch, designs[:3] + [designs[3] * 2.0], filter_index=[0, 1, 2, 0])
    # the C entry point itself: an error through vfx_last_error, y untouched
    dbl = ctypes.POINTER(ctypes.c_double)
    y = torch.full((4, 500), 5.0, dtype=torch.float64, device=DEV)

    def call(lengths, index, sections=(1, 2, 2, 5), padlens=(9, 12, 15, 33), Smax=5, scale=1.0, ldy=500):
        sos = np.zeros((4, Smax, 6))
        sos[..., 0] = sos[..., 3] = 1.0
        for f, d in enumerate(designs):
            sos[f, :d.shape[0]] = d * scale
        zi = np.zeros((4, Smax, 2))
        return eng.lib.vfx_sosfiltfilt_bank(eng.h, ctypes.c_void_p(batch.data_ptr()), 0, 4, 500, (ctypes.c_int64 * 4)(*lengths),
                                            (ctypes.c_int * 4)(*index), sos.ctypes.data_as(dbl), zi.ctypes.data_as(dbl),
                                            (ctypes.c_int * 4)(*sections), (ctypes.c_int * 4)(*padlens), 4, Smax,
                                            ctypes.c_void_p(y.data_ptr()), ldy, None)
    assert call([500, 20, 20, 20], [0, 3, 1, 2]) != 0
    err = eng.lib.vfx_last_error()
    assert b"clip 1 " in err and b"20 samples" in err and b"which is 33" in err
    assert call([500, 500, 500, 500], [0, 4, 1, 2]) != 0 and b"clip 1 asks for design 4 of 4" in eng.lib.vfx_last_error()
    assert call([500, 500, 500, 500], [0, -1, 1, 2]) != 0
    assert call([500, 500, 500, 500], [0, 1, 2, 3], Smax=17) != 0 and b"17 sections" in eng.lib.vfx_last_error()
    assert call([500, 500, 500, 500], [0, 1, 2, 3], sections=(1, 2, 6, 5)) != 0 and b"6 sections" in eng.lib.vfx_last_error()
    assert call([500, 500, 500, 500], [0, 1, 2, 3], scale=2.0) != 0 and b"should be 1" in eng.lib.vfx_last_error()
    assert call([500, 501, 500, 500], [0, 1, 2, 3]) != 0
    for ldy in (499, -1):      # a row stride of y that does not hold the clips, a negative one included
        assert call([500, 500, 500, 500], [0, 1, 2, 3], ldy=ldy) != 0 and b"the rows hold 500 and %d" % ldy in eng.lib.vfx_last_error()
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())
    with pytest.raises(RuntimeError, match="which is 33"):
        _lib.check(call([500, 20, 20, 20], [0, 3, 1, 2]), "vfx_sosfiltfilt_bank")


def test_lowpass_each_equals_lowpass(eng):
    """24 clips, cut-offs 750 .. 16 000 Hz, orders 2 .. 10, all six types -- "stft" at 1000 Hz (the device resampler takes it) and at
    1234 Hz (it does not), one "stft_hard" --, float32 with a few float64 clips: every item is `lowpass` of that clip alone."""
    from voicefixer_main_amd import simulate
    rng = np.random.default_rng(24)
    types = ["cheby1", "ellip", "bessel", "butter"] * 5 + ["stft", "stft", "stft_hard", "stft"]
    highcuts = [int(v) for v in rng.integers(750, 16001, 24)]
    highcuts[20], highcuts[21], highcuts[23] = 1000, 1234, 1000
    orders = [int(v) for v in rng.integers(2, 11, 24)]
    order = [int(v) for v in rng.permutation(24)]
    types, highcuts, orders = ([v[i] for i in order] for v in (types, highcuts, orders))
    clips = [rng.uniform(-1, 1, int(n)).astype(np.float64 if i % 7 == 3 else np.float32) for i, n in enumerate(rng.integers(2000, 3001, 24))]
    assert eng.resample_supported(FS, 2000) and not eng.resample_supported(FS, int(1234 / int(FS / 2) * FS))
    want = [simulate.lowpass(c, h, FS, o, t, engine=eng) for c, h, o, t in zip(clips, highcuts, orders, types)]
    got = simulate.lowpass_each(clips, highcuts, FS, orders, types, engine=eng)
    dev = simulate.lowpass_each(clips, highcuts, FS, orders, types, engine=eng, to_host=False)
    for i, (w, g, d) in enumerate(zip(want, got, dev)):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w), (i, types[i], highcuts[i], orders[i])
        assert d.device.type == "cuda" and np.array_equal(d.cpu().numpy(), w), (i, types[i])


def test_bandpass_each_equals_bandpass(eng):
    from voicefixer_main_amd import simulate
    rng = np.random.default_rng(8)
    clips = [rng.uniform(-1, 1, int(n)).astype(np.float64 if i == 2 else np.float32) for i, n in enumerate(rng.integers(500, 3001, 8))]
    lowcuts = [int(v) for v in rng.integers(100, 2000, 8)]
    highcuts = [int(v) for v in rng.integers(3000, 12000, 8)]
    orders = [2, 3, 5, 10, 7, 10, 4, 14]
    types = ["butter", "cheby1", "ellip", "cheby1", "bessel", "butter", "b", "ellip"]
    got = simulate.bandpass_each(clips, lowcuts, highcuts, FS, orders, types, engine=eng)
    for i, (c, lc, hc, o, t) in enumerate(zip(clips, lowcuts, highcuts, orders, types)):
        want = simulate.bandpass(c, lc, hc, FS, o, t)
        assert np.isfinite(want).all() and got[i].dtype == want.dtype and np.array_equal(got[i], want), (i, t, o)


def test_lowpass_collate_equals_the_single_clip_loop(eng):
    """A seeded 6-item batch against a plain loop over the single-clip host functions that consumes an identically seeded generator
    in the collator's order (data_module.py:28-70)."""
    from voicefixer_main_amd import simulate
    L, lo, hi, o_lo, o_hi = 4410, 1500, 44100, 2, 10
    types = ["cheby1", "ellip", "bessel", "stft_hard", "stft", "butter"]
    data = np.random.default_rng(6)
    batch = [{"fname": "item%d" % i, "vocals": data.uniform(-1, 1, (L, 1)).astype(np.float32),
              "vocals_aug": data.uniform(-1, 1, (L, 1)).astype(np.float32), "noise": data.uniform(-1, 1, (L, 1)).astype(np.float32)}
             for i in range(6)]
    got = simulate.lowpass_collate(batch, [lo, hi], [o_lo, o_hi], types, FS, rng=np.random.default_rng(66), engine=eng)

    rng = np.random.default_rng(66)

    def uniform(lower, upper):
        return (upper - lower) * rng.random() + lower

    def lowpass(x, c, o, f):
        return simulate.lowpass(x, highcut=c, fs=FS, order=o, _type=f, engine=eng)

    cutoffs, orders, filters = [], [], []
    for _ in batch:
        cutoffs.append(int(uniform(lo // 2, hi // 2)))
        orders.append(int(uniform(o_lo, o_hi)))
        filters.append(types[int(uniform(0, len(types)))])
    want = {}
    for key in ("vocals", "vocals_aug"):
        want[key] = []
        for x, c, o, f in zip(batch, cutoffs, orders, filters):
            chance = uniform(0, 1000)
            y = lowpass(x[key][..., 0], c, o, f)
            want[key].append(lowpass(y, c, o, "stft") if int(chance) % 2 == 0 else y)
    want["noise"] = []
    for x, c, o, f in zip(batch, cutoffs, orders, filters):
        chance = uniform(0, 1000)
        if int(chance) % 2 == 0:
            want["noise"].append(x["noise"][..., 0])
            continue
        y = lowpass(x["noise"][..., 0], c, o, f)
        want["noise"].append(lowpass(y, c, o, "stft") if int(chance) % 3 == 0 else y)

    assert got["fname"] == ["item%d" % i for i in range(6)]
    for key, rows in want.items():
        assert got[key].device.type == "cuda" and got[key].dtype == torch.float32 and got[key].shape == (6, L, 1)
        assert got[key + "_LR"].device.type == "cuda" and got[key + "_LR"].dtype == torch.float32 and got[key + "_LR"].shape == (6, L, 1)
        for i, w in enumerate(rows):
            assert np.array_equal(got[key][i, :, 0].cpu().numpy(), batch[i][key][:, 0]), (key, i)
            assert np.array_equal(got[key + "_LR"][i, :, 0].cpu().numpy(), w.astype(np.float32)), (key, i, filters[i], cutoffs[i], orders[i])
    host = simulate.lowpass_collate(batch, [lo, hi], [o_lo, o_hi], types, FS, rng=np.random.default_rng(66), engine=eng, to_host=True)
    assert all(host[k].device.type == "cpu" and torch.equal(host[k], got[k].cpu()) for k in got if k != "fname")
