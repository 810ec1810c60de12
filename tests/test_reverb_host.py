"""Host side of the RIR convolution: simulate.reverb_rir against the reference's formula written out with SciPy, synth.make_rir, and
the binding of vfx_reverb_rir.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, simulate, synth  # noqa: E402


def _formula(frames, rir):
    """MagicalEffects.reverb_rir (dataloaders/augmentation/magical_effects.py:158-167), step by step"""
    n = frames.shape[0]
    full = signal.convolve(np.squeeze(frames), np.squeeze(rir))
    peak = np.max(np.abs(full))
    if peak > 0.99:
        full = (full / peak) * 0.98
    return full[:n], peak


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("gain, scaled", [(0.05, False), (1.0, True)])
def test_reverb_rir_is_the_reference_formula(dtype, gain, scaled):
    rng = np.random.default_rng(1)
    x = (rng.uniform(-1, 1, 4000) * gain).astype(dtype)
    h = synth.make_rir(3, 900).astype(dtype)
    want, peak = _formula(x, h)
    assert (peak > 0.99) == scaled
    y = simulate.reverb_rir(x, h)
    assert y.dtype == dtype and y.shape == (4000,) and np.array_equal(y, want)
    if scaled:      # the peak of the FULL result is 0.98: the cut may have removed it, it cannot exceed it
        assert np.abs(y).max() <= dtype(0.98) * (1 + 4 * np.finfo(dtype).eps)


def test_reverb_rir_shapes():
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, 300)
    h = synth.make_rir(4, 120)
    y = simulate.reverb_rir(x, h)
    # (N, 1) frames and a (1, M) RIR are squeezed; the result has the first N samples
    assert np.array_equal(simulate.reverb_rir(x[:, None], h[None, :]), y) and y.shape == (300,)
    # a RIR longer than the clip: the peak is taken over all N + M - 1 samples, the cut keeps N
    long_h = synth.make_rir(5, 1000).astype(np.float64) * 3.0
    want, peak = _formula(x, long_h)
    assert peak > 0.99 and want.shape == (300,)
    assert np.array_equal(simulate.reverb_rir(x, long_h), want)
    # an impulse at the last sample: only tap 0 lands inside the clip, the tail sets the peak
    e = np.zeros(100)
    e[99] = 1.0
    taps = np.zeros(50)
    taps[0], taps[49] = 0.5, 2.0
    y = simulate.reverb_rir(e, taps)
    assert y[99] == 0.5 / 2.0 * 0.98 and not y[:99].any()
    # integers go through as SciPy takes them
    assert np.array_equal(simulate.reverb_rir(np.array([1, 2, 3]), np.array([1, 1])), np.array([1, 3, 5]) / 5 * 0.98)


def test_make_rir():
    a, b = synth.make_rir(7, 5000), synth.make_rir(7, 5000)
    assert a.dtype == np.float32 and a.shape == (5000,) and np.array_equal(a, b)
    assert not np.array_equal(a, synth.make_rir(8, 5000))
    assert a[0] == 1.0 and np.abs(a[1:]).max() < 1.0                      # the direct path dominates
    assert np.abs(a[-500:]).mean() < np.abs(a[100:600]).mean()            # and the tail decays
    assert synth.make_rir(7, 1).tolist() == [1.0]


def test_signature_matches_the_header():
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert re.search(r"\bint\s+vfx_reverb_rir\s*\(", header)
    res, args = _lib.SIGNATURES["vfx_reverb_rir"]
    i64p = ctypes.POINTER(ctypes.c_int64)
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, i64p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                    i64p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    decl = re.search(r"int\s+vfx_reverb_rir\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(args)


def test_reverb_rir_list_checks_its_index():
    with pytest.raises(ValueError):
        simulate.reverb_rir_list([np.zeros(10)], [np.ones(3)], rir_index=[1], engine=object())
    with pytest.raises(ValueError):
        simulate.reverb_rir_list([np.zeros(10)], [], engine=object())
