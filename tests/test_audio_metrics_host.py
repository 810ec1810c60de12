"""CPU: the float64 restatement of AudioMetrics' scores, aggregate_score / gather_score with a stub scorer, and score.hip's assembly."""
import csv
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_metrics_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_restatement_reproduces_the_reference_metric_outputs():
    """LSD and SiSpec of the restatement (per clip) against what the reference's own functions returned (tests/golden/metrics.npz)."""
    g = np.load(os.path.join(G, "metrics.npz"))
    for tag in "abc":
        e, t = g[tag + "_est"].astype(np.float64), g[tag + "_tgt"].astype(np.float64)
        lsd = np.array([ref.lsd(e[b, 0], t[b, 0]) for b in range(e.shape[0])])
        np.testing.assert_allclose(lsd, g[tag + "_lsd"][:, 0, 0, 0], rtol=1e-5)
        lin = np.mean([ref.sispec(e[b, 0], t[b, 0]) for b in range(e.shape[0])])
        log = np.mean([ref.sispec(ref.to_log(e[b, 0]), ref.to_log(t[b, 0])) for b in range(e.shape[0])])
        assert abs(lin - float(g[tag + "_sispec_lin"])) < 2e-3
        assert abs(log - float(g[tag + "_sispec_log"])) < 2e-3


@pytest.mark.parametrize("shape", [(7, 7), (9, 12), (15, 8), (7, 20)])
def test_ssim_uniform_filter_matches_window_loop(shape):
    rng = np.random.default_rng(sum(shape))
    x = 10.0 ** rng.normal(-1.0, 0.8, size=shape)
    y = x * (1.0 + 0.3 * rng.normal(size=shape))
    assert abs(ref.ssim(x, y) - ref.ssim_brute(x, y)) < 1e-12
    assert abs(ref.ssim(x, x) - 1.0) < 1e-12


@pytest.mark.parametrize("shape", [(6, 10), (10, 6)])
def test_ssim_refuses_images_below_the_window(shape):
    with pytest.raises(ValueError):
        ref.ssim(np.ones(shape), np.ones(shape))
    from voicefixer_main_amd.metrics import AudioMetrics
    m = AudioMetrics.__new__(AudioMetrics)
    with pytest.raises(ValueError):
        m.ssim(torch.ones((1, 1) + shape), torch.ones((1, 1) + shape))


def test_sisdr_is_scale_invariant_and_saturates_at_eps():
    rng = np.random.default_rng(3)
    t = rng.normal(size=5000)
    e = t + 0.1 * rng.normal(size=5000)
    assert abs(ref.sisdr(3.7 * e, t) - ref.sisdr(e, t)) < 1e-9
    assert abs(ref.sisdr(e, t) - 20.0) < 1.0
    # identical signals: Snn = 0, the score is the eps ceiling 10 log10((eps + |t|^2) / eps)
    eps = np.finfo(np.float64).eps
    assert abs(ref.sisdr(t, t) - 10 * np.log10((eps + np.dot(t, t)) / eps)) < 1e-9


def test_audio_metrics_keys_and_rate():
    from voicefixer_main_amd import metrics
    assert metrics.METRIC_KEYS == ref.KEYS
    assert len(metrics.METRIC_KEYS) == 9
    with pytest.raises(ValueError, match="Bad Samplerate"):
        metrics.AudioMetrics(16000, engine=StubEngine())
    assert metrics.AudioMetrics(44100, engine=StubEngine()).evaluation("x.wav", None) == {}


def test_c_abi_declares_audio_metrics():
    from voicefixer_main_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert re.search(r"#define VFX_N_AUDIO_METRICS 9\b", hdr) and _lib.N_AUDIO_METRICS == 9
    assert "vfx_audio_metrics" in _lib.SIGNATURES and re.search(r"\bvfx_audio_metrics\(", hdr)


# ----------------------------------------------------------------------------------------------------------------------
# aggregate_score / gather_score with a stub in place of the engine
# ----------------------------------------------------------------------------------------------------------------------
class StubEngine:
    """audio_metrics on the host by the float64 restatement; records the batches it is handed."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def audio_metrics(self, est, target, lengths):
        self.calls.append(list(lengths))
        e, t = est.numpy(), target.numpy()
        return torch.from_numpy(np.stack([ref.audio_metrics(e[b, :n], t[b, :n]) for b, n in enumerate(lengths)]))


def _save(path, x):
    from voicefixer_main_amd import handlers
    handlers.save_wave(x, path)


def _pcm(x):
    return (np.asarray(x, np.float64) * 2 ** 15).astype(np.short).astype(np.float32) / 32768.0


def _testset(tmp_path, name, lines, files):
    d = tmp_path / "data" / name
    d.mkdir(parents=True, exist_ok=True)
    for fname, x in files.items():
        _save(str(d / fname), x)
    lst = tmp_path / (name + ".lst")
    lst.write_text("".join(l.replace("@", str(d) + "/") + "\n" for l in lines))
    return {"rate": 44100, "list": str(lst)}


def test_aggregate_score_writes_json_csv_and_result(tmp_path):
    from voicefixer_main_amd import metrics, synth
    rng = np.random.default_rng(5)
    clean = {"c%d.wav" % i: synth.speech_like(n, 40 + i) * 0.5 for i, n in enumerate((9000, 4410, 6000, 7000))}
    noisy = {"n%d.wav" % i: x + 0.05 * rng.normal(size=x.shape) for i, x in enumerate(clean.values())}
    lines = ["@n0.wav @c0.wav", "@n1.wav @c1.wav", "@n2.wav", "@n3.wav @c3.wav", "@n2.wav @c2.wav"]
    meta = {"set_a": _testset(tmp_path, "set_a", lines, {**clean, **noisy})}
    save = tmp_path / "out"
    (save / "set_a").mkdir(parents=True)
    # restored files: n0 and n1 as the "handler" wrote them, n3 missing (a failing pair), n2 as well
    ests = {}
    for i in (0, 1, 2):
        x = list(clean.values())[i] * 0.9 + 0.01 * rng.normal(size=list(clean.values())[i].shape)
        _save(str(save / "set_a" / ("n%d.wav" % i)), x)
        ests[i] = _pcm(x)
    (save / "set_a" / "n0.json").write_text(json.dumps({"mel-lsd": 1.5, "sisdr": -99.0}))
    stub = StubEngine()
    out = metrics.aggregate_score(str(save), ["set_a"], metas=meta, engine=stub)
    rows = out["set_a"]
    assert list(rows) == ["c0.wav", "c1.wav", "c2.wav"]              # n3 failed and is left out; the one-field line is skipped
    assert sorted(sum(stub.calls, [])) == [4410, 6000, 9000] and stub.calls[0] == sorted(stub.calls[0])
    for i, name in enumerate(rows):
        want = ref.audio_metrics(ests[i], _pcm(list(clean.values())[i]))
        js = json.loads((save / "set_a" / ("n%d.json" % i)).read_text())
        assert js == rows[name]
        for k, v in zip(ref.KEYS, want):
            if not (i == 0 and k == "sisdr"):
                assert abs(js[k] - v) < 1e-9 * max(1.0, abs(v)), (name, k)
    assert rows["c0.wav"]["sisdr"] == -99.0 and rows["c0.wav"]["mel-lsd"] == 1.5     # the handler's JSON wins, as score_part_2.update
    with open(save / "set_a" / "set_a.csv") as f:
        table = list(csv.reader(f))
    assert table[0][0] == "" and table[0][1:10] == list(ref.KEYS) and table[0][10] == "mel-lsd"
    assert [r[0] for r in table[1:]] == ["c0.wav", "c1.wav", "c2.wav", "mean"]
    res = json.loads((save / "set_a" / "result.json").read_text())
    for j, k in enumerate(table[0][1:]):
        have = [rows[n][k] for n in rows if k in rows[n]]
        assert abs(res[k] - np.mean(have)) < 1e-12 and abs(float(table[-1][j + 1]) - res[k]) < 1e-12
    assert table[-2][10] == ""                                          # c2 has no handler JSON: empty cell, not in the mean
    assert res["mel-lsd"] == 1.5
    # limit_number: only the first line of the list
    stub2 = StubEngine()
    out = metrics.aggregate_score(str(save), ["set_a"], limit_number=1, metas=meta, engine=stub2)
    assert list(out["set_a"]) == ["c0.wav"] and stub2.calls == [[9000]]
    # gather_score: one row per test set with a result.json
    meta["set_b"] = _testset(tmp_path, "set_b", ["@n1.wav"], {})
    metrics.aggregate_score(str(save), ["set_b"], metas=meta, engine=StubEngine())
    assert not (save / "set_b" / "result.json").exists()
    got = metrics.gather_score(str(save), ["set_a", "set_b"])
    assert list(got) == ["set_a"]
    with open(save / "result.csv") as f:
        table = list(csv.reader(f))
    assert [r[0] for r in table] == ["", "set_a"]


def test_evaluation_list_reports_errors_per_pair(tmp_path):
    from voicefixer_main_amd import metrics, synth
    x = synth.speech_like(5000, 1) * 0.5
    a, b, short, other = (str(tmp_path / n) for n in ("a.wav", "b.wav", "short.wav", "other.wav"))
    _save(a, x)
    _save(b, x[::-1].copy())
    _save(short, x[:2645])
    _save(other, x[:4000])
    m = metrics.AudioMetrics(44100, engine=StubEngine())
    r = m.evaluation_list([(a, b), (short, short), (a, other), (a, str(tmp_path / "missing.wav"))])
    assert isinstance(r[0], dict) and list(r[0]) == list(ref.KEYS)
    assert isinstance(r[1], ValueError) and isinstance(r[2], ValueError) and isinstance(r[3], Exception)
    with pytest.raises(ValueError):
        m.evaluation(a, other)


# ----------------------------------------------------------------------------------------------------------------------
# score.hip on gfx950: no spills, no FLAT memory operations, clean under both assembly checkers
# ----------------------------------------------------------------------------------------------------------------------
def test_score_kernels_assembly_is_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "score.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", out, os.path.join(ROOT, "voicefixer_main_amd", "csrc", "score.hip")],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    kernels = dict(re.findall(r"\n(_ZN3vfx\w+):.*?; ScratchSize: (\d+)", asm, re.S))
    for name in ("k_sisdr_slabs", "k_score_frames", "k_ssim_tiles", "k_score_final"):
        assert any(name in k for k in kernels), (name, list(kernels))
    for k, scratch in kernels.items():
        assert int(scratch) == 0, (k, scratch)
    assert not re.search(r"\n\s*flat_(load|store|atomic)", asm)
    for checker in ("asm_store_hazard_check.py", "asm_inflight_check.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", checker), out], capture_output=True, text=True)
        assert r.returncode == 0, (checker, r.stdout[-2000:])
