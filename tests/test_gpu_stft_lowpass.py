"""GPU: the fused "stft_hard" low-pass (Engine.stft_lowpass, k_stft_lowpass in csrc/stft.hip) -- every clip of a padded batch bit for
bit what the two-launch path (simulate.stft_hard_lowpass_v0: vfx_stft_mel, the mask and the two products by torch, vfx_istft) gives for
it alone, in the small-launch geometry (IH = 2) and the large one (IH = 16), zeros past a clip's length; against the float64 oracle;
the list forms of simulate built on it; and the argument checks of vfx_stft_lowpass."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, clips as _clips, simulate  # noqa: E402

pytestmark = pytest.mark.gpu

FS = 44100
HOP = 441
NBINS = 1025
# 1025: the shortest clip the reflection allows; 1323 = 3 * 441; 1764 / 1765: an overlap-add group of 2 * 441 ends inside the clip and
# one sample later; 4410 + 123
SMALL_LENGTHS = [1025, 1323, 1764, 1765, 2048, 2500, 4410 + 123]
# 46: what 1000 Hz gives; 64: the lane boundary; 1024 / 1025 straddle the bin lane 0 handles alone; 2000: no mask
SMALL_CUTS = [0, 1, 46, 64, 1024, 1025, 2000]


@pytest.fixture(scope="module")
def eng():
    from voicefixer_main_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Engine("cuda:0")


def _clip(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def _ratio(cut):
    """A ratio with int(1025 * ratio) == cut, the expression of stft_hard_lowpass_v0"""
    r = (cut + 0.5) / NBINS
    assert int(NBINS * r) == cut
    return r


def _reference(eng, clips, cuts):
    return [simulate.stft_hard_lowpass_v0(c, _ratio(k), engine=eng) for c, k in zip(clips, cuts)]


@pytest.fixture(scope="module")
def small(eng):
    """The small batch: clips, and each one's own two-launch result (computed once, shared, never written)"""
    clips = [_clip(n, 100 + i) for i, n in enumerate(SMALL_LENGTHS)]
    return clips, _reference(eng, clips, SMALL_CUTS)


def _run(eng, clips, cuts):
    lengths = [c.shape[0] for c in clips]
    y = eng.stft_lowpass(_clips.pad(clips, eng.device, torch.float32), cuts, lengths=lengths)
    assert y.dtype == torch.float32 and y.shape == (len(clips), max(lengths)) and y.device == eng.device
    return y.cpu().numpy()


def _assert_rows(y, want, lengths):
    for b, (w, n) in enumerate(zip(want, lengths)):
        assert w.dtype == np.float32 and w.shape == (n,)
        assert np.array_equal(y[b, :n], w), (b, n, float(np.abs(y[b, :n] - w).max()))
        assert not y[b, n:].any(), (b, n)


def test_small_batch_bit_identical_per_clip(eng, small):
    clips, want = small
    assert len(clips) * eng.frames(max(SMALL_LENGTHS)) < 4096      # the launch with IH = 2
    y = _run(eng, clips, SMALL_CUTS)
    _assert_rows(y, want, SMALL_LENGTHS)
    assert not y[0].any()      # cut = 0
    assert all(w.any() for w in want[1:])
    assert eng.take_flags() == 0
    # a 1-D clip, a scalar cut
    one = eng.stft_lowpass(torch.from_numpy(clips[3]), SMALL_CUTS[3])
    assert one.shape == (SMALL_LENGTHS[3],) and np.array_equal(one.cpu().numpy(), want[3])


def test_large_batch_bit_identical_per_clip(eng):
    rng = np.random.default_rng(7)
    lengths = [int(v) for v in rng.integers(1025, 14201, size=128)]
    lengths[5] = max(lengths[5], 13671 + 17)
    edge = 16 * HOP - 1024      # the first sample the second overlap-add group of 16 hops owns
    lengths[40], lengths[41] = edge - 1, edge + 1
    cuts = [int(v) for v in rng.integers(0, 1101, size=128)]
    B, T = len(lengths), eng.frames(max(lengths))
    assert max(lengths) >= 13671 and T >= 32 and B * T >= 4096      # the launch with IH = 16
    clips = [_clip(n, 1000 + i) for i, n in enumerate(lengths)]
    y = _run(eng, clips, cuts)
    _assert_rows(y, _reference(eng, clips, cuts), lengths)
    assert eng.take_flags() == 0


def test_against_float64(eng, small):
    """The bound tests/test_simulate.py holds `stft_hard` to."""
    from oracle import dsp
    clips, _ = small
    pick = [SMALL_CUTS.index(k) for k in (46, 64, 1025)]
    y = _run(eng, [clips[i] for i in pick], [SMALL_CUTS[i] for i in pick])
    for row, i in zip(y, pick):
        x, cut = clips[i], SMALL_CUTS[i]
        mag, cos, sin = dsp.spectrogram_phase(x[None, None].astype(np.float64), dtype=np.float64)
        mag[..., cut:] = 0.0
        ref = dsp.istft((mag * cos)[0], (mag * sin)[0], x.shape[0], dtype=np.float64)[0]
        err = float(np.abs(row[:x.shape[0]] - ref).max())
        print("cut %d, %d samples: max |got - ref| = %.3g, max |ref| = %.3g" % (cut, x.shape[0], err, np.abs(ref).max()))
        assert err < 2e-5 * max(1.0, np.abs(ref).max()), (cut, err)


def _equal(got, want, device=None):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if device is not None:
            assert isinstance(g, torch.Tensor) and g.device == device
            g = g.cpu().numpy()
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def test_lowpass_list_is_the_loop_over_lowpass(eng, small):
    clips, _ = small
    want = [simulate.lowpass(c, 4000, FS, _type="stft_hard", engine=eng) for c in clips]
    _equal(simulate.lowpass_list(clips, 4000, FS, _type="stft_hard", engine=eng), want)
    _equal(simulate.lowpass_list(clips, 4000, FS, _type="stft_hard", engine=eng, to_host=False), want, eng.device)


def test_lowpass_each_is_the_loop_over_lowpass(eng):
    lengths = [3000, 1025, 2205, 4410, 1500, 2048, 1323, 3500, 1100, 2600, 1765, 5000]
    clips = [_clip(n, 300 + i) for i, n in enumerate(lengths)]
    for i in (1, 4, 9):      # float64 clips: one of each kind of type
        clips[i] = clips[i].astype(np.float64)
    types = ["stft_hard", "butter", "stft", "stft_hard"] * 3
    assert len(clips) == 12 and {types[i] for i in (1, 4, 9)} == {"butter", "stft_hard"} and types[2] == "stft"
    clips[2] = clips[2].astype(np.float64)      # ... and a float64 "stft" item
    highcuts = [1000, 4000, 11025, 8000, 2000, 3000, 1000, 22050, 12000, 6000, 11025, 500]
    want = [simulate.lowpass(c, h, FS, _type=t, engine=eng) for c, h, t in zip(clips, highcuts, types)]
    _equal(simulate.lowpass_each(clips, highcuts, FS, types=types, engine=eng), want)
    _equal(simulate.lowpass_each(clips, highcuts, FS, types=types, engine=eng, to_host=False), want, eng.device)
    assert eng.take_flags() == 0


def test_argument_checks_launch_nothing(eng):
    """A clip too short for the reflection, a negative cut and `out` aliasing `wav`: each an error of the entry point."""
    B, L = 2, 2048
    wav = torch.zeros((B, L), device=eng.device)
    out = torch.full((B, L), 7.0, device=eng.device)
    ints = ctypes.c_int * B
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def call(lengths, cuts, dst):
        rc = eng.lib.vfx_stft_lowpass(eng.h, P(wav), B, L, ints(*lengths), ints(*cuts), P(dst), eng._stream())
        return rc, (_lib.load().vfx_last_error() or b"").decode()

    rc, msg = call([2048, 1024], [10, 10], out)
    assert rc != 0 and "clip 1 has 1024 samples" in msg
    rc, msg = call([2048, 2049], [10, 10], out)
    assert rc != 0 and "clip 1 has 2049 samples" in msg
    rc, msg = call([2048, 2048], [10, -1], out)
    assert rc != 0 and "cut-off bin -1" in msg
    rc, msg = call([2048, 2048], [10, 10], wav)
    assert rc != 0 and "overlaps wav" in msg
    with pytest.raises(RuntimeError, match="1024 samples"):
        eng.stft_lowpass(wav[:, :1024], 10)
    torch.cuda.synchronize(eng.device)
    assert bool((out == 7.0).all())      # nothing ran
    rc, _ = call([2048, 2048], [10, 10], out)
    assert rc == 0 and not bool(out.any())      # the low-pass of silence
