"""CPU: the float64 restatement of STOI (tests/stoi_f64.py) against the facts of the published algorithm, and the host side of
vfx_stoi: the filter Engine.stoi builds, the `stoi=` switch of AudioMetrics / aggregate_score with a stub engine, the C ABI."""
import csv
import json
import os
import re

import numpy as np
import pytest
import torch

import audio_metrics_f64 as ref9
import stoi_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(n, seed):
    return np.random.default_rng(seed).normal(size=n)


def test_identical_signals_score_one():
    from voicefixer_main_amd import synth
    for x in (_noise(6000, 1), synth.speech_like(10000, 3, sr=10000)):
        assert abs(ref.stoi(x, x) - 1.0) < 1e-12
    x = synth.speech_like(44100, 4).astype(np.float32)
    assert abs(ref.stoi(x, x, 44100) - 1.0) < 1e-12


def test_band_edges():
    assert ref.band_edges() == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69),
                                (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]


def test_octave_filter_lengths():
    assert ref.ratio(44100) == (100, 441) and ref.ratio(16000) == (5, 8)
    assert ref.filter_half_length(100, 441) == 15973 and len(ref.resample_filter(100, 441)) == 31947
    assert ref.filter_half_length(5, 8) == 290 and len(ref.resample_filter(5, 8)) == 581
    taps = ref.resample_taps(5, 8)
    assert abs(taps.sum() - 5.0) < 1e-12 and np.array_equal(taps, taps[::-1])


def test_resample_is_the_plain_polyphase_sum():
    """y[o] = sum_k x[k] taps[L + o down - k up]: the sum k_stoi_resample restates, and the per-output terms of its bound."""
    x = _noise(700, 8)
    up, down = 5, 8
    taps, L = ref.resample_taps(up, down), ref.filter_half_length(up, down)
    y = ref.resample(x, 16000)
    K, mag = ref.resample_terms(x, up, down)
    assert len(y) == -(-700 * up // down) == len(K) == len(mag)
    for o in (0, 1, 17, 200, len(y) - 1):
        k = np.arange(len(x))
        j = L + o * down - k * up
        ok = (j >= 0) & (j < len(taps))
        terms = x[ok] * taps[j[ok]]
        assert K[o] == ok.sum()
        assert abs(mag[o] - np.abs(terms).sum()) <= 1e-12 * mag[o]
        assert abs(y[o] - terms.sum()) <= (K[o] + 2) * 2.0 ** -53 * mag[o]


@pytest.mark.parametrize("n,kept,frames,segments", [(3969, 30, 29, 0), (4097, 31, 30, 1), (4225, 32, 31, 2)])
def test_frame_counts_at_the_30_frame_boundary(n, kept, frames, segments):
    t = _noise(n, n)
    e = t + 0.5 * _noise(n, n + 1)
    mask = ref.keep_mask(t)
    assert mask.sum() == kept == len(mask)
    es, ts = ref.remove_silent_frames(e, t)
    assert len(ts) == (kept - 1) * 128 + 256 == len(es)
    assert ref.tob(ts).shape == (15, frames)
    d = ref.stoi(e, t)
    if segments == 0:
        assert d == 1e-5
    else:
        assert 0.3 < d < 1.0
        assert max(0, frames - 29) == segments


def test_shorter_than_one_frame_scores_the_short_value():
    assert ref.stoi(np.ones(200), np.ones(200)) == 1e-5
    assert ref.stoi(np.ones(256), np.ones(256)) == 1e-5


def test_zero_signals_score_zero_without_nan():
    t = _noise(8000, 5)
    z = np.zeros(8000)
    assert ref.stoi(z, t) == 0.0
    assert ref.stoi(t, z) == 0.0


def test_score_is_not_symmetric():
    from voicefixer_main_amd import synth
    t = synth.speech_like(10000, 11, sr=10000)
    e = np.clip(t + 0.3 * _noise(10000, 12), -0.4, 0.4)
    assert abs(ref.stoi(e, t) - ref.stoi(t, e)) > 1e-3


def test_score_falls_with_snr():
    from voicefixer_main_amd import synth
    t = synth.speech_like(10000, 21, sr=10000)
    nz = _noise(10000, 22)
    nz *= np.sqrt(np.mean(t ** 2) / np.mean(nz ** 2))
    d = [ref.stoi(t + nz * 10.0 ** (-snr / 20.0), t) for snr in (30, 10, 0, -10)]
    assert all(a > b for a, b in zip(d, d[1:])), d
    assert d[0] > 0.9, d


def test_silent_frames_are_joined():
    """Exact-zero gaps at both ends and in the middle: their frames go, and kept frames that were not neighbours are overlap-added."""
    t = _noise(6000, 31)
    t[:700] = 0.0
    t[2500:3400] = 0.0
    t[5300:] = 0.0
    mask = ref.keep_mask(t)
    assert 0 < mask.sum() < len(mask) and not mask[0] and not mask[-1] and not mask[22]
    e, s = ref.remove_silent_frames(0.5 * t, t)
    assert len(s) == (mask.sum() - 1) * 128 + 256
    np.testing.assert_array_equal(e, 0.5 * s)


# ----------------------------------------------------------------------------------------------------------------------
# the host side of the package
# ----------------------------------------------------------------------------------------------------------------------
def test_engine_builds_the_restatements_filter():
    from voicefixer_main_amd.engine import Engine

    class Host(Engine):   # stoi_taps needs the device only to place the filter
        def __init__(self):
            self.device = torch.device("cpu")
            self._stoi_taps = {}

    h = Host()
    for fs, (up, down) in ((44100, (100, 441)), (16000, (5, 8))):
        u, d, taps, ntaps = h.stoi_taps(fs)
        assert (u, d) == (up, down) and ntaps == 2 * ref.filter_half_length(up, down) + 1
        assert taps.dtype == torch.float64 and np.array_equal(taps.numpy(), ref.resample_taps(up, down))
        assert h.stoi_taps(fs)[2] is taps                                   # cached per (up, down)
    assert h.stoi_taps(10000) == (1, 1, None, 0)
    u, d, taps, ntaps = h.stoi_taps(44101)                                  # too long to build: left to the library to refuse
    assert taps is None and ntaps > 1 << 20


class StubEngine:
    """audio_metrics / stoi on the host by the float64 restatements; records what it is handed."""
    device = torch.device("cpu")

    def __init__(self, with_stoi=True):
        self.batches, self.stoi_batches = [], []
        if with_stoi:
            self.stoi = self._stoi

    def audio_metrics(self, est, target, lengths):
        self.batches.append((est, target, list(lengths)))
        e, t = est.numpy(), target.numpy()
        return torch.from_numpy(np.stack([ref9.audio_metrics(e[b, :n], t[b, :n]) for b, n in enumerate(lengths)]))

    def _stoi(self, est, target, lengths=None, fs=44100):
        self.stoi_batches.append((est, target, list(lengths), fs))
        e, t = est.numpy(), target.numpy()
        return torch.tensor([ref.stoi(e[b, :n], t[b, :n], fs) for b, n in enumerate(lengths)], dtype=torch.float64)


def _pcm(x):
    return (np.asarray(x, np.float64) * 2 ** 15).astype(np.short).astype(np.float32) / 32768.0


def _files(tmp_path):
    from voicefixer_main_amd import handlers, synth
    rng = np.random.default_rng(5)
    d = tmp_path / "data"
    d.mkdir()
    pairs, sig = [], []
    for i, n in enumerate((44100, 52000, 48000)):
        clean = synth.speech_like(n, 60 + i) * 0.5
        noisy = clean + 0.05 * rng.normal(size=n)
        handlers.save_wave(clean, str(d / ("c%d.wav" % i)))
        handlers.save_wave(noisy, str(d / ("n%d.wav" % i)))
        pairs.append((str(d / ("n%d.wav" % i)), str(d / ("c%d.wav" % i))))
        sig.append((_pcm(noisy), _pcm(clean)))
    return pairs, sig


def test_audio_metrics_keys_with_and_without_stoi(tmp_path):
    from voicefixer_main_amd import metrics
    pairs, sig = _files(tmp_path)
    plain = metrics.AudioMetrics(44100, engine=StubEngine(with_stoi=False))
    assert plain.keys == metrics.METRIC_KEYS and len(metrics.METRIC_KEYS) == 9
    for r in plain.evaluation_list(pairs):
        assert tuple(r) == metrics.METRIC_KEYS
    stub = StubEngine()
    judge = metrics.AudioMetrics(44100, engine=stub, stoi=True)
    assert judge.keys == ("sisdr", "stoi") + metrics.METRIC_KEYS[1:]
    res = judge.evaluation_list(pairs)
    for r, r9, (e, t) in zip(res, plain.evaluation_list(pairs), sig):
        assert tuple(r) == judge.keys and len(r) == 10
        assert {k: r[k] for k in r9} == r9
        assert abs(r["stoi"] - ref.stoi(e, t, 44100)) < 1e-12 and 0.3 < r["stoi"] < 1.0
    # one vfx_stoi call per padded batch, on the very tensors audio_metrics was handed: no second upload
    assert len(stub.batches) == len(stub.stoi_batches) == 1
    (e9, t9, l9), (e1, t1, l1, fs) = stub.batches[0], stub.stoi_batches[0]
    assert e9 is e1 and t9 is t1 and l9 == l1 and fs == 44100
    assert tuple(judge.evaluation(*pairs[0])) == judge.keys


def test_aggregate_score_carries_the_stoi_column(tmp_path):
    from voicefixer_main_amd import metrics
    pairs, sig = _files(tmp_path)
    save = tmp_path / "out"
    (save / "set_a").mkdir(parents=True)
    lines = []
    for est, tgt in pairs:
        os.replace(est, str(save / "set_a" / os.path.basename(est)))
        lines.append("%s %s" % (est, tgt))
    (tmp_path / "a.lst").write_text("\n".join(lines) + "\n")
    metas = {"set_a": {"rate": 44100, "list": str(tmp_path / "a.lst")}}
    rows = metrics.aggregate_score(str(save), ["set_a"], metas=metas, engine=StubEngine(), stoi=True)["set_a"]
    want = [ref.stoi(e, t, 44100) for e, t in sig]
    assert [abs(rows["c%d.wav" % i]["stoi"] - w) < 1e-12 for i, w in enumerate(want)] == [True] * 3
    with open(save / "set_a" / "set_a.csv") as f:
        table = list(csv.reader(f))
    assert table[0][1:3] == ["sisdr", "stoi"] and len(table[0]) == 11
    res = json.loads((save / "set_a" / "result.json").read_text())
    assert abs(res["stoi"] - np.mean(want)) < 1e-12 and abs(float(table[-1][2]) - res["stoi"]) < 1e-15


def test_c_abi_declares_stoi():
    from voicefixer_main_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert "vfx_stoi" in _lib.SIGNATURES and re.search(r"\bint vfx_stoi\(", hdr)
    assert len(_lib.SIGNATURES["vfx_stoi"][1]) == 12
    test_hdr = open(os.path.join(ROOT, "include", "vfx_test.h")).read()
    assert "vfx_op_stoi_stage" in _lib.TEST_SIGNATURES and re.search(r"\bint vfx_op_stoi_stage\(", test_hdr)
    assert re.search(r"#define VFX_N_AUDIO_METRICS 9\b", hdr) and _lib.N_AUDIO_METRICS == 9
    mk = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bstoi\.hip\b", mk, re.M)
