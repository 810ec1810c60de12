"""Host side of the batched "stft_hard" low-pass: the binding of vfx_stft_lowpass, and how simulate's list forms hand their clips to
Engine.stft_lowpass -- sorted by length, float32, at most 128 per call, a cut-off bin per clip, results in the caller's order; short
clips and engines without the method take the single-clip function.  A recording stub stands in for the Engine.  No GPU."""
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, simulate  # noqa: E402

FS = 44100
HEAD = 8      # the stub's "spectrum" is made of a clip's first samples


def test_signature_matches_the_header():
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert re.search(r"\bint\s+vfx_stft_lowpass\s*\(", header)
    res, args = _lib.SIGNATURES["vfx_stft_lowpass"]
    decl = re.search(r"int\s+vfx_stft_lowpass\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(args) == 8


class PerClip:
    """stft / istft alone, as the fake engines of the other host tests have them: 1025 bins made of the clip's first samples."""
    device = torch.device("cpu")

    def __init__(self):
        self.stft_calls = []      # lengths of the clips that came through the single-clip function

    def stft(self, x, want_mel, want_sp, want_phase):
        assert x.dtype == torch.float32 and x.shape[0] == 1
        self.stft_calls.append(x.shape[1])
        w = torch.linspace(1.0, 2.0, 1025)
        sp = x[:, :HEAD, None].abs() * w
        return dict(sp=sp, cos=torch.sign(x[:, :HEAD, None]) * torch.ones(1025), sin=torch.zeros_like(sp))

    def istft(self, re, im, length):
        y = torch.zeros((re.shape[0], length))
        n = min(HEAD, length)
        y[:, :n] = re.sum(-1)[:, :n]
        return y


class Batched(PerClip):
    """... plus stft_lowpass, on the host by looping the stub's own stft / istft, recording what it was handed."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def stft_lowpass(self, x, cut_bins, lengths=None):
        self.calls.append(dict(shape=tuple(x.shape), dtype=x.dtype, cut_bins=list(cut_bins), lengths=list(lengths)))
        y = torch.zeros_like(x)
        seen = len(self.stft_calls)
        for b, (n, cut) in enumerate(zip(lengths, cut_bins)):
            o = self.stft(x[b:b + 1, :n], want_mel=False, want_sp=True, want_phase=True)
            sp = o["sp"]
            sp[..., cut:] = 0.0
            y[b, :n] = self.istft(sp * o["cos"], sp * o["sin"], n)[0]
        del self.stft_calls[seen:]      # (only the single-clip path is counted)
        return y


def _clips(lengths, seed=5, f64=()):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, n).astype(np.float64 if i in f64 else np.float32) for i, n in enumerate(lengths)]


def test_lowpass_list_hands_over_sorted_float32_batches_of_at_most_128():
    lengths = [1025 + (37 * i) % 130 for i in range(130)]      # 130 distinct lengths, not in order
    assert len(set(lengths)) == 130 and lengths != sorted(lengths)
    lengths[7], lengths[90] = 1024, 300      # too short for the reflection: the single-clip function
    clips = _clips(lengths, f64=(3, 64))
    highcut = 4000
    eng = Batched()
    got = simulate.lowpass_list(clips, highcut, FS, _type="stft_hard", engine=eng)
    long = sorted(n for n in lengths if n > 1024)
    assert [c["lengths"] for c in eng.calls] == [long[:128]]
    assert eng.calls[0]["shape"] == (128, long[127]) and eng.calls[0]["dtype"] == torch.float32
    cut = int(1025 * (highcut / int(FS / 2)))
    assert cut == 185 and eng.calls[0]["cut_bins"] == [cut] * 128
    assert sorted(eng.stft_calls) == [300, 1024]
    ref = PerClip()
    want = [simulate.lowpass(c, highcut, FS, _type="stft_hard", engine=ref) for c in clips]
    assert len({w[:HEAD].tobytes() for w in want}) == len(want)      # no two results alike: the order is checked
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and np.array_equal(g, w)
    # more than 128 long clips: a second call for the longest
    eng = Batched()
    clips = _clips([1025 + i for i in range(131)][::-1])
    got = simulate.lowpass_list(clips, highcut, FS, _type="stft_hard", engine=eng, to_host=False)
    assert [len(c["lengths"]) for c in eng.calls] == [128, 3] and eng.calls[1]["lengths"] == [1153, 1154, 1155] and eng.stft_calls == []
    assert eng.calls[1]["shape"] == (3, 1155)
    for g, c in zip(got, clips):
        assert isinstance(g, torch.Tensor) and np.array_equal(g.numpy(), simulate.lowpass(c, highcut, FS, _type="stft_hard", engine=ref))


def test_lowpass_each_hands_over_a_cut_per_clip():
    lengths = [2000, 1025, 1500, 1024, 1100]
    clips = _clips(lengths, seed=9, f64=(2,))
    highcuts = [1000, 4000, 22050, 8000, 30000]
    eng = Batched()
    got = simulate.lowpass_each(clips, highcuts, FS, types="stft_hard", engine=eng)
    cut = lambda h: int(1025 * (h / int(FS / 2)))      # noqa: E731
    assert [cut(h) for h in highcuts] == [46, 185, 1025, 371, 1394]
    assert eng.calls == [dict(shape=(4, 2000), dtype=torch.float32, cut_bins=[cut(4000), cut(30000), cut(22050), cut(1000)],
                              lengths=[1025, 1100, 1500, 2000])]
    assert eng.stft_calls == [1024]
    ref = PerClip()
    for g, c, h in zip(got, clips, highcuts):
        assert g.dtype == np.float32 and np.array_equal(g, simulate.lowpass(c, h, FS, _type="stft_hard", engine=ref))


def test_a_negative_cut_and_an_engine_without_the_method_take_the_single_clip_function():
    clips = _clips([1500, 1200, 1300], seed=11)
    eng = Batched()
    got = simulate.lowpass_each(clips, [4000, -4000, 500], FS, types="stft_hard", engine=eng)
    assert [c["lengths"] for c in eng.calls] == [[1300, 1500]] and eng.stft_calls == [1200]
    ref = PerClip()
    for g, c, h in zip(got, clips, [4000, -4000, 500]):
        assert np.array_equal(g, simulate.lowpass(c, h, FS, _type="stft_hard", engine=ref))
    plain = PerClip()
    got = simulate.lowpass_list(clips, 4000, FS, _type="stft_hard", engine=plain)
    assert plain.stft_calls == [1500, 1200, 1300]
    for g, c in zip(got, clips):
        assert np.array_equal(g, simulate.lowpass(c, 4000, FS, _type="stft_hard", engine=ref))
