"""Host side of the batched noise mixers: the binding of vfx_mix_noise, and the list forms of simulate on clips that take the host
path -- equal to a loop over the single-clip functions, the same draws from the generator, no Engine.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, simulate  # noqa: E402

FORMS = [      # (list form, single-clip form, signals)
    (simulate.add_noise_and_scale_list, simulate.add_noise_and_scale, 2),
    (simulate.add_noise_and_scale_with_HQ_list, simulate.add_noise_and_scale_with_HQ, 3),
    (simulate.add_noise_and_scale_with_HQ_with_Aug_list, simulate.add_noise_and_scale_with_HQ_with_Aug, 4),
]


def test_signature_matches_the_header():
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert re.search(r"\bint\s+vfx_mix_noise\s*\(", header)
    res, args = _lib.SIGNATURES["vfx_mix_noise"]
    vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int
    assert args == [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), vp, vp, vp, vp, dp, dp,
                    vp, vp, vp, vp, vp, vp]
    decl = re.search(r"int\s+vfx_mix_noise\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(args)


def _no_engine(monkeypatch):
    def boom():
        raise AssertionError("the host path must not create an Engine")
    monkeypatch.setattr(simulate, "_get_engine", boom)


def _signals(nsig, lengths, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(n) * rng.uniform(0.05, 1.5)).astype(dtype) for n in lengths] for _ in range(nsig)]


@pytest.mark.parametrize("list_fn, one_fn, nsig", FORMS)
@pytest.mark.parametrize("with_snr", [True, False])
def test_host_path_is_the_loop_over_the_single_clip_function(monkeypatch, list_fn, one_fn, nsig, with_snr):
    _no_engine(monkeypatch)
    lengths = [1, 7, 300, 64, 1000]
    sig = _signals(nsig, lengths, seed=nsig)
    kw = dict(snr_l=-5 if with_snr else None, snr_h=30, scale_lower=0.5, scale_upper=0.9)
    a, b = np.random.default_rng(77), np.random.default_rng(77)
    got = list_fn(*sig, rng=a, want_noisy=True, **kw)
    assert len(got) == len(lengths)
    for i in range(len(lengths)):
        want = one_fn(*[s[i] for s in sig], rng=b, **kw)
        assert len(got[i]) == len(want) + 1
        for g, w in zip(got[i][:nsig], want[:nsig]):
            assert g.dtype == np.float64 and np.array_equal(g, w)
        assert got[i][nsig] == want[nsig] and got[i][nsig + 1] == want[nsig + 1]      # snr, scale
        assert (got[i][nsig] is None) == (not with_snr)
        # noisy: the noise (last signal) + the speech it was mixed into (the one before it)
        assert np.array_equal(got[i][-1], want[nsig - 1] + want[nsig - 2])
    assert a.random() == b.random()      # the generator is where the loop left it
    plain = list_fn(*sig, rng=np.random.default_rng(77), **kw)
    assert all(len(t) == nsig + 2 for t in plain) and np.array_equal(plain[2][0], got[2][0])


def test_constant_draws_and_integer_clips(monkeypatch):
    """an (almost) empty interval draws nothing (_uniform); integer clips go as NumPy takes them"""
    _no_engine(monkeypatch)
    front, noise = [np.array([1, -2, 3])], [np.array([2, 0, -1])]
    a = np.random.default_rng(5)
    (f, n, snr, scale), = simulate.add_noise_and_scale_list(front, noise, snr_l=10, snr_h=10, scale_lower=0.7, scale_upper=0.7, rng=a)
    wf, wn, wsnr, wscale = simulate.add_noise_and_scale(front[0], noise[0], snr_l=10, snr_h=10, scale_lower=0.7, scale_upper=0.7)
    assert np.array_equal(f, wf) and np.array_equal(n, wn) and (snr, scale) == (wsnr, wscale) == (10, 0.7)
    assert a.random() == np.random.default_rng(5).random()


@pytest.mark.parametrize("list_fn, one_fn, nsig", FORMS)
def test_errors(monkeypatch, list_fn, one_fn, nsig):
    _no_engine(monkeypatch)
    sig = _signals(nsig, [50, 60], seed=3)
    sig[-1][1] = sig[-1][1][:59]                      # the noise of item 1 is one sample short
    with pytest.raises(ValueError, match="item 1"):
        list_fn(*sig, rng=np.random.default_rng(0))
    sig = _signals(nsig, [50, 60], seed=3)
    sig[0][0] = sig[0][0][:, None]                    # (samples, 1)
    with pytest.raises(ValueError, match="item 0"):
        list_fn(*sig, rng=np.random.default_rng(0))
    sig = _signals(nsig, [50, 60], seed=3, dtype=np.float32)      # float32 clips are checked before anything runs, too
    sig[1][0] = sig[1][0][:49]
    with pytest.raises(ValueError, match="item 0"):
        list_fn(*sig, rng=np.random.default_rng(0))
    with pytest.raises(ValueError):
        list_fn(*[s[:1] if k == 0 else s for k, s in enumerate(_signals(nsig, [50, 60], seed=3))])      # lists of unequal length


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hard_clip_list(monkeypatch, dtype):
    _no_engine(monkeypatch)
    rng = np.random.default_rng(9)
    clips = [(rng.standard_normal(n) * 0.5).astype(dtype) for n in (1, 33, 1000)]
    clips[1][5] = np.nan
    got = simulate.hard_clip_list(clips, 0.25)
    for g, c in zip(got, clips):
        want = simulate.hard_clip(c, 0.25)
        assert g.dtype == want.dtype == dtype and np.array_equal(g, want, equal_nan=True)
        assert np.nanmax(np.abs(g)) <= dtype(0.25)
