"""CPU: the float64 restatement of BSS Eval (tests/bsseval_f64.py) against closed forms, the conditions the inputs of
tests/test_gpu_bsseval.py are held to -- shown on the reference alone --, planted defects that the GPU test's 1e-9 dB must be able to
see, and the host side of vfx_bsseval: the `bsseval=` switch of AudioMetrics / aggregate_score with a stub engine, the C ABI."""
import csv
import json
import os
import re

import numpy as np
import pytest
import torch

import audio_metrics_f64 as ref9
import bsseval_f64 as ref
import stoi_f64 as ref_stoi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slab():
    from voicefixer_main_amd import _lib
    return _lib.BSSEVAL_SLAB


# ----------------------------------------------------------------------------------------------------------------------
# the restatement against closed forms
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen,k,g", [(16, 3, 0.5), (48, 47, -1.25), (512, 100, 0.8)])
def test_a_scaled_delay_is_one_tap(flen, k, g):
    """est = g x the target delayed by k < flen, no noise: the filter is g at tap k, isr is the closed form of that P, and sdr is the
    plain energy ratio."""
    n = 3000
    r = np.random.default_rng(11).standard_normal(n).astype(np.float32)
    e = np.zeros(n, np.float32)
    e[k:] = (np.float32(g) * r[:n - k])
    a, d = ref.correlations(e, r, flen)
    c = ref.solve_lu(a, d)
    # the est is cut at n, so the fit is g at tap k up to the edge effect of the k lost samples
    assert abs(c[k] - g) < 0.05 and np.abs(np.delete(c, k)).max() < 0.05
    P = ref.project(c, r)
    r64 = np.zeros(n + flen - 1)
    r64[:n] = r
    sdr, isr, sar = ref.bsseval(e, r, flen)
    assert abs(isr - 10 * np.log10(np.sum(r64 ** 2) / np.sum((P - r64) ** 2))) < 1e-12
    assert abs(sdr - 10 * np.log10(np.sum(r.astype(np.float64) ** 2) / np.sum((e.astype(np.float64) - r) ** 2))) < 1e-12
    assert sar > 15.0                                           # (what the filter cannot explain is only the cut tail)


def test_identical_signals_and_silence():
    x = np.random.default_rng(12).standard_normal(700).astype(np.float32)
    sdr, isr, sar = ref.bsseval(x, x, 48)
    assert sdr == np.inf and isr > 200.0 and sar > 200.0
    z = np.zeros(700, np.float32)
    assert np.all(np.isnan(ref.bsseval(z, x, 48))) and np.all(np.isnan(ref.bsseval(x, z, 48)))
    assert ref.scores([1.0, 0.0, 0.0, 2.0, 0.0]).tolist() == [np.inf] * 3


def test_the_two_correlations_and_the_two_solvers_agree():
    e, r = ref.make_a(700, 1)
    a, d = ref.correlations(e, r, 48)
    af, df = ref.correlations_fft(e, r, 48)
    assert np.abs(a - af).max() < 1e-10 and np.abs(d - df).max() < 1e-10
    assert a[0] == np.sum(r.astype(np.float64) ** 2) and abs(d[5] - np.sum(e[5:].astype(np.float64) * r[:-5])) < 1e-12
    assert np.abs(ref.solve_lu(a, d) - ref.solve_levinson(a, d)).max() < 1e-12
    exact, mag, cnt = ref.correlation_terms(e, r, 48)
    assert np.abs(exact[0] - a).max() < 1e-10 and cnt[1, 47] == 700 - 47 and np.all(mag >= np.abs(exact))


# ----------------------------------------------------------------------------------------------------------------------
# the conditions on the GPU test's inputs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", ref.FLENS)
def test_the_gpu_cases_are_well_conditioned(flen):
    """For every (maker, seed, n, flen) of tests/test_gpu_bsseval.py: cond(toeplitz(a)) <= 1e4, the three scores finite and below
    100 dB, and (LU, direct sums) within 1e-10 dB of (Levinson, FFT correlations): the scores are defined four to five orders
    below the 1e-9 dB the device is held to."""
    for maker, seed, n, f in ref.cases(_slab()):
        if f != flen:
            continue
        e, r = ref.pair(maker, seed, n)
        a, _ = ref.correlations(e, r, flen)
        cond = np.linalg.cond(ref.toeplitz(a))
        sc = ref.bsseval(e, r, flen)
        spread = ref.solver_spread(e, r, flen)
        assert cond <= 1e4, (maker, seed, n, flen, cond)
        assert np.all(np.isfinite(sc)) and np.all(sc < 100.0), (maker, seed, n, flen, sc)
        assert spread <= 1e-10, (maker, seed, n, flen, spread)


def test_the_quiet_gpu_cases_are_well_conditioned():
    """The same conditions for input A at the level where the eps of the definition counts (bsseval_f64.QUIET_CASES), and that it
    does count there: it is more than 1e-6 of a[0]."""
    for seed, n, flen in ref.QUIET_CASES:
        e, r = ref.quiet_pair(seed, n)
        assert np.array_equal(e, ref.make_a(n, seed)[0] * np.float32(ref.QUIET))      # the unit-level samples, another exponent
        a, _ = ref.correlations(e, r, flen)
        sc = ref.bsseval(e, r, flen)
        assert ref.EPS > 1e-6 * a[0] and np.linalg.cond(ref.toeplitz(a)) <= 1e4 and np.linalg.cond(ref.gram(a)) <= 1e4
        assert np.all(np.isfinite(sc)) and np.all(sc < 100.0), (n, flen, sc)
        assert ref.solver_spread(e, r, flen) <= 1e-10, (n, flen)


# ----------------------------------------------------------------------------------------------------------------------
# planted defects: each must move a score of input A by more than 1e-6 dB, three orders above the GPU test's tolerance
# ----------------------------------------------------------------------------------------------------------------------
def _scores_with(e, r, flen, d_sign=1, eps=True, energy_len=None, p_len=None):
    e, r = np.asarray(e, np.float64), np.asarray(r, np.float64)
    n = len(r)
    a, d = ref.correlations(e, r, flen)
    if d_sign < 0:      # d[k] = sum e[t] r[t + k]
        d = np.array([np.dot(e[:n - k], r[k:]) if k < n else 0.0 for k in range(flen)])
    G = ref.toeplitz(a) + (ref.EPS if eps else 0.0) * np.eye(flen)
    P = ref.project(np.linalg.solve(G, d), r)
    if p_len is not None:
        P = np.concatenate([P[:p_len], np.zeros(len(P) - p_len)])
    m = len(P) if energy_len is None else energy_len
    rp, ep = np.zeros(len(P)), np.zeros(len(P))
    rp[:n], ep[:n] = r, e
    return ref.scores(ref.energies(ep[:m], rp[:m], P[:m]))


PLANTED_N, PLANTED_FLEN, PLANTED_SEED = 700, 48, 1


def _moved(scale=1.0, **defect):
    e, r = ref.make_a(PLANTED_N, PLANTED_SEED, scale)
    good = _scores_with(e, r, PLANTED_FLEN)
    assert np.array_equal(good, ref.bsseval(e, r, PLANTED_FLEN))
    return float(np.max(np.abs(_scores_with(e, r, PLANTED_FLEN, **defect) - good)))


def test_planted_wrong_lag_sign_is_seen():
    assert _moved(d_sign=-1) > 1e-6


def test_planted_energies_over_n_are_seen():
    assert _moved(energy_len=PLANTED_N) > 1e-6


def test_planted_truncated_projection_is_seen():
    assert _moved(p_len=PLANTED_N) > 1e-6


def test_planted_missing_eps_is_seen():
    """On input A at unit level the eps decides nothing: a[0] = sum r^2 = 659.7 here, 2^-52 is under half an ulp of it, toeplitz(a) +
    2^-52 I is toeplitz(a) bit for bit and the scores move by exactly 0.0 dB.  The eps is absolute and the rest of the definition
    scales with the level, so the defect is planted where it can show: the same input A at 2^-24 of that level (bsseval_f64.QUIET),
    which tests/test_gpu_bsseval.py scores on the device for that reason."""
    assert _moved(eps=False) == 0.0
    assert _moved(scale=ref.QUIET, eps=False) > 1e-6
    for seed, n, flen in ref.QUIET_CASES:                            # every quiet case of the GPU test sees it
        e, r = ref.quiet_pair(seed, n)
        assert np.max(np.abs(_scores_with(e, r, flen, eps=False) - ref.bsseval(e, r, flen))) > 1e-6, (n, flen)


# ----------------------------------------------------------------------------------------------------------------------
# the host side of the package
# ----------------------------------------------------------------------------------------------------------------------
class StubEngine:
    """audio_metrics / stoi / bsseval on the host by the float64 restatements; records what it is handed."""
    device = torch.device("cpu")

    def __init__(self, silent=()):
        self.batches, self.stoi_batches, self.bss_batches = [], [], []
        self.silent = set(silent)           # lengths whose pair is scored as a silent one: NaN x 3

    def audio_metrics(self, est, target, lengths):
        self.batches.append((est, target, list(lengths)))
        e, t = est.numpy(), target.numpy()
        return torch.from_numpy(np.stack([ref9.audio_metrics(e[b, :n], t[b, :n]) for b, n in enumerate(lengths)]))

    def stoi(self, est, target, lengths=None, fs=44100):
        self.stoi_batches.append((est, target, list(lengths), fs))
        e, t = est.numpy(), target.numpy()
        return torch.tensor([ref_stoi.stoi(e[b, :n], t[b, :n], fs) for b, n in enumerate(lengths)], dtype=torch.float64)

    def bsseval(self, est, target, lengths=None, flen=512):
        self.bss_batches.append((est, target, list(lengths), flen))
        e, t = est.numpy(), target.numpy()
        rows = [np.full(3, np.nan) if n in self.silent else ref.bsseval(e[b, :n], t[b, :n], 48) for b, n in enumerate(lengths)]
        return torch.from_numpy(np.stack(rows))


def _pcm(x):
    return (np.asarray(x, np.float64) * 2 ** 15).astype(np.short).astype(np.float32) / 32768.0


LENGTHS = (3000, 3400, 3200)


def _files(tmp_path):
    from voicefixer_main_amd import handlers
    rng = np.random.default_rng(5)
    d = tmp_path / "data"
    d.mkdir()
    pairs, sig = [], []
    for i, n in enumerate(LENGTHS):
        clean = 0.2 * rng.standard_normal(n)
        noisy = 0.7 * clean + 0.05 * rng.standard_normal(n)
        handlers.save_wave(clean, str(d / ("c%d.wav" % i)))
        handlers.save_wave(noisy, str(d / ("n%d.wav" % i)))
        pairs.append((str(d / ("n%d.wav" % i)), str(d / ("c%d.wav" % i))))
        sig.append((_pcm(noisy), _pcm(clean)))
    return pairs, sig


def test_audio_metrics_keys_with_and_without_bsseval(tmp_path):
    from voicefixer_main_amd import metrics
    assert metrics.BSSEVAL_KEYS == ("sdr", "isr", "sar")
    pairs, sig = _files(tmp_path)
    plain = metrics.AudioMetrics(44100, engine=StubEngine())
    assert plain.keys == metrics.METRIC_KEYS
    off = metrics.AudioMetrics(44100, engine=StubEngine(), bsseval=False)
    assert off.keys == metrics.METRIC_KEYS and off.evaluation_list(pairs) == plain.evaluation_list(pairs)
    stub = StubEngine()
    judge = metrics.AudioMetrics(44100, engine=stub, bsseval=True)
    assert judge.keys == metrics.METRIC_KEYS + ("sdr", "isr", "sar")
    for r, r9, (e, t) in zip(judge.evaluation_list(pairs), plain.evaluation_list(pairs), sig):
        assert tuple(r) == judge.keys and len(r) == 12
        assert {k: r[k] for k in r9} == r9
        assert [r[k] for k in ref.KEYS] == ref.bsseval(e, t, 48).tolist()
    # one vfx_bsseval call per padded batch, on the very tensors audio_metrics was handed: no second upload
    assert len(stub.batches) == len(stub.bss_batches) == 1 and not stub.stoi_batches
    (e9, t9, l9), (e1, t1, l1, flen) = stub.batches[0], stub.bss_batches[0]
    assert e9 is e1 and t9 is t1 and l9 == l1 and flen == 512
    both = metrics.AudioMetrics(44100, engine=StubEngine(), stoi=True, bsseval=True)
    assert both.keys == ("sisdr", "stoi") + metrics.METRIC_KEYS[1:] + ("sdr", "isr", "sar")
    assert tuple(both.evaluation(*pairs[0])) == both.keys


def test_aggregate_score_carries_the_bsseval_columns(tmp_path):
    from voicefixer_main_amd import metrics
    pairs, sig = _files(tmp_path)

    def run(name, **kw):
        save = tmp_path / name
        (save / "set_a").mkdir(parents=True)
        lines = []
        for est, tgt in pairs:
            with open(est, "rb") as f:
                (save / "set_a" / os.path.basename(est)).write_bytes(f.read())
            lines.append("%s %s" % (est, tgt))
        (tmp_path / (name + ".lst")).write_text("\n".join(lines) + "\n")
        metas = {"set_a": {"rate": 44100, "list": str(tmp_path / (name + ".lst"))}}
        rows = metrics.aggregate_score(str(save), ["set_a"], metas=metas, **kw)["set_a"]
        with open(save / "set_a" / "set_a.csv") as f:
            table = list(csv.reader(f))
        return rows, table, (save / "set_a" / "result.json").read_text()

    rows0, table0, res0 = run("plain", engine=StubEngine())
    rows1, table1, res1 = run("off", engine=StubEngine(), bsseval=False)
    assert rows0 == rows1 and table0 == table1 and res0 == res1 and len(table0[0]) == 10          # what it is today
    # the pair of 3400 samples scores NaN (a silent est or target): skipped in the three means, as pandas does
    rows, table, res = run("on", engine=StubEngine(silent=(3400,)), bsseval=True)
    assert table[0] == table0[0] + ["sdr", "isr", "sar"]
    assert [row[:10] for row in table] == table0                                                  # no other column changes
    res, res0 = json.loads(res), json.loads(res0)
    assert {k: res[k] for k in res0} == res0
    want = np.array([ref.bsseval(e, t, 48) for (e, t), n in zip(sig, LENGTHS) if n != 3400])
    for j, k in enumerate(ref.KEYS):
        assert np.isnan(rows["c1.wav"][k]) and rows["c0.wav"][k] == want[0, j]
        assert abs(res[k] - want[:, j].mean()) < 1e-12 and float(table[-1][10 + j]) == res[k]


def test_c_abi_declares_bsseval():
    from voicefixer_main_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vfx.h")).read()
    assert "vfx_bsseval" in _lib.SIGNATURES and re.search(r"\bint vfx_bsseval\(", hdr)
    assert len(_lib.SIGNATURES["vfx_bsseval"][1]) == 9
    test_hdr = open(os.path.join(ROOT, "include", "vfx_test.h")).read()
    assert "vfx_op_bsseval_stage" in _lib.TEST_SIGNATURES and re.search(r"\bint vfx_op_bsseval_stage\(", test_hdr)
    assert len(_lib.TEST_SIGNATURES["vfx_op_bsseval_stage"][1]) == 11
    assert re.search(r"#define VFX_BSSEVAL_SLAB %d\b" % _lib.BSSEVAL_SLAB, hdr)
    mk = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bbsseval\.hip\b", mk, re.M)
