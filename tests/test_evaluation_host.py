"""CPU: evaluation.inference's routing rule with a stub model that records its calls -- which files are batched, which fall back to the
per-file handler, in which order --, list lines with and without a target, the wav and JSON paths, limit_number."""
import json
import os
import wave

import numpy as np
import pytest
import torch


def _write(path, n, rate=44100, seed=0):
    x = (np.random.default_rng(seed).uniform(-0.5, 0.5, size=n) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(x.tobytes())
    return x.astype(np.float32) / 32768.0


class StubModel:
    """restore_list / restore_scored_list of a model: halves every clip, scores it by its length"""
    device = torch.device("cpu")
    engine = None

    def __init__(self):
        self.calls = []

    def restore_scored_list(self, wavs, targets, unify_energy=False, max_batch=128):
        self.calls.append(("scored", [int(w.shape[0]) for w in wavs], [int(t.shape[0]) for t in targets], unify_energy, max_batch))
        return [w * 0.5 for w in wavs], [{"mel-lsd": float(w.shape[0]), "mel-ssim": float(t.shape[0])} for w, t in zip(wavs, targets)]

    def restore_list(self, wavs, unify_energy=False, max_batch=128):
        self.calls.append(("plain", [int(w.shape[0]) for w in wavs], unify_energy, max_batch))
        return [w * 0.5 for w in wavs]


@pytest.fixture
def testset(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    clips = {}
    spec = [("a", 20000, 20010, 44100), ("b", 20000, 21000, 44100), ("c", 5000, None, 44100), ("d", 1000, None, 44100),
            ("e", 20000, 20000, 22050), ("f", 2000, 2000, 44100), ("g", 44100 * 60 + 1, None, 44100), ("i", 2646, 3086, 44100),
            ("j", 44100 * 60, None, 44100)]
    lines = []
    for k, (name, n, m, rate) in enumerate(spec):
        clips[name] = _write(d / ("noisy_%s.wav" % name), n, rate, seed=k)
        if m is not None:
            _write(d / ("clean_%s.wav" % name), m, 44100 if name != "e" else 22050, seed=100 + k)
        lines.append(str(d / ("noisy_%s.wav" % name)) + ("" if m is None else " " + str(d / ("clean_%s.wav" % name))))
    lines.insert(3, str(d / "missing.wav") + " " + str(d / "clean_a.wav"))       # h: a file that is not there
    (tmp_path / "set.lst").write_text("\n".join(lines) + "\n")
    return tmp_path, lines, clips


def _run(tmp_path, **kw):
    from voicefixer_main_amd import evaluation
    model = StubModel()
    fell = []

    def handler(input, output, target, ckpt, device, needrefresh, meta):
        fell.append((os.path.basename(input), None if target is None else os.path.basename(target), meta.get("unify_energy")))
        with open(output, "wb") as f:
            f.write(b"handler")
        return {"from": "handler"} if target is not None else {}

    metas = {"demo": {"rate": 44100, "list": str(tmp_path / "set.lst"), "unify_energy": True}}
    evaluation.inference(model, str(tmp_path / "out"), ["demo"], metas, handler=handler, **kw)
    return model, fell


def test_routing_order_and_paths(testset):
    from voicefixer_main_amd import handlers
    tmp_path, lines, clips = testset
    model, fell = _run(tmp_path)
    # batched: a and i (one segment, a target of the input's frame count and >= 2646 samples), c and j (no target, one segment)
    assert model.calls == [("scored", [20000, 2646], [20010, 3086], True, 128), ("plain", [5000, 44100 * 60], True, 128)]
    # everything else goes to the handler, in list order: frame-count mismatch, a missing file, <= 1024 samples, another rate, a
    # target below 2646 samples, longer than one segment
    assert fell == [("noisy_b.wav", "clean_b.wav", True), ("missing.wav", "clean_a.wav", True), ("noisy_d.wav", None, True),
                    ("noisy_e.wav", "clean_e.wav", True), ("noisy_f.wav", "clean_f.wav", True), ("noisy_g.wav", None, True)]
    out = tmp_path / "out" / "demo"
    names = sorted(os.listdir(out))
    stems = ["missing"] + ["noisy_%s" % c for c in "abcdefgij"]
    assert names == sorted([s + ".wav" for s in stems] + [s + ".json" for s in stems])
    # a batched file is the model's clip through save_wave, its JSON the model's scores; {} without a target
    for name, scores in (("a", {"mel-lsd": 20000.0, "mel-ssim": 20010.0}), ("i", {"mel-lsd": 2646.0, "mel-ssim": 3086.0}), ("c", {})):
        handlers.save_wave(clips[name] * 0.5, str(tmp_path / "want.wav"))
        assert (out / ("noisy_%s.wav" % name)).read_bytes() == (tmp_path / "want.wav").read_bytes()
        assert json.loads((out / ("noisy_%s.json" % name)).read_text()) == scores
    for name, scores in (("b", {"from": "handler"}), ("d", {}), ("g", {})):
        assert (out / ("noisy_%s.wav" % name)).read_bytes() == b"handler"
        assert json.loads((out / ("noisy_%s.json" % name)).read_text()) == scores


def test_limit_number_and_windows(testset, monkeypatch):
    from voicefixer_main_amd import evaluation
    tmp_path, lines, _ = testset
    model, fell = _run(tmp_path, limit_number=3)
    assert model.calls == [("scored", [20000], [20010], True, 128), ("plain", [5000], True, 128)]
    assert [f[0] for f in fell] == ["noisy_b.wav"]
    assert sorted(os.listdir(tmp_path / "out" / "demo")) == sorted(s + e for s in ("noisy_a", "noisy_b", "noisy_c") for e in (".wav", ".json"))
    # a long list is read and restored a window of WINDOW_BATCHES * max_batch lines at a time, still in list order
    monkeypatch.setattr(evaluation, "WINDOW_BATCHES", 2)
    model, fell = _run(tmp_path, max_batch=2, limit_number=9)
    assert model.calls == [("scored", [20000], [20010], True, 2), ("plain", [5000], True, 2), ("scored", [2646], [3086], True, 2)]
    assert [f[0] for f in fell] == ["noisy_b.wav", "missing.wav", "noisy_d.wav", "noisy_e.wav", "noisy_f.wav", "noisy_g.wav"]


def test_is_batched_rule(testset):
    from voicefixer_main_amd import evaluation
    tmp_path, _, _ = testset
    d = tmp_path / "data"
    p = lambda s: str(d / s)
    assert evaluation.is_batched(p("noisy_a.wav"), p("clean_a.wav")) and evaluation.is_batched(p("noisy_a.wav"), None)
    assert not evaluation.is_batched(p("noisy_a.wav"), p("clean_b.wav"))          # 46 frames against 48
    assert not evaluation.is_batched(p("noisy_d.wav"), None) and not evaluation.is_batched(p("noisy_g.wav"), None)
    assert evaluation.is_batched(p("noisy_j.wav"), None)                            # exactly 60 s is one segment
    assert not evaluation.is_batched(p("noisy_f.wav"), p("clean_f.wav")) and evaluation.is_batched(p("noisy_f.wav"), None)
    assert not evaluation.is_batched(p("noisy_e.wav"), None) and not evaluation.is_batched(p("nothing.wav"), None)
    _write(d / "short_target.wav", 1025)
    _write(d / "short_input.wav", 1100)
    assert not evaluation.is_batched(p("short_input.wav"), p("short_target.wav"))   # same frame count, below 2646 samples


def test_scored_sets_are_single_process(monkeypatch):
    from voicefixer_main_amd import dist as vdist, models
    monkeypatch.setattr(vdist, "world_rank", lambda: (2, 0))
    with pytest.raises(RuntimeError, match="one process"):
        models._restore_scored_list(None, None, [], [], 8, None, None, "restore_scored_list")
