"""CPU: streaming sessions without a GPU -- the NumPy model of a session (tests/stream_ref.py) against the chunker oracle for seeded
blockings, the released counts after every feed, planted defects, and the library's own scheduler (stream_sched.cpp) driven by a
stand-alone program under AddressSanitizer + UBSan, whose printed schedule must be the model's line for line.

Shapes, lengths and block sizes are the issue's.  Tolerances against the oracle: 2e-6 (overlap-add) and 1e-6 (boxcar), those of
test_chunkers_vs_reference_golden at these sizes.  For the boxcar mode the block sizes' "H" is max(in_margin, 2).

oracle.overlap_add_boxcar cannot be evaluated at in_margin = 0: its `[..., :-M]` / `[..., M:-M]` slices are empty there.  At
that margin the model is held against `_boxcar_without_margin`, the same function with those slices read as "cut M samples".
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import stream_ref as sr
from oracle import chunker as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voicefixer_main_amd", "csrc")

OLA_SHAPES = [(126, 21), (64, 16), (64, 32), (64, 64)]
BOX_SHAPES = [(126, 7), (64, 0), (64, 8)]
CASES = [(sr.OLA, W, H, win) for W, H in OLA_SHAPES for win in ("hanning", None)] + \
        [(sr.BOXCAR, W, M, win) for W, M in BOX_SHAPES for win in ("hanning", None)]
IDS = ["%s-%d-%d-%s" % ("ola" if m == sr.OLA else "box", W, P, win) for m, W, P, win in CASES]


def _lengths(W):
    return [5, W - 1, W, 3 * W, 1237]      # 0 < L < W twice, L = W, L = kW, 1237


def _boxcar_without_margin(x, W, win):
    """overlapadd_boxcar.py:420-513 at in_margin = 0: frames of W samples, the first zero-padded to W, a ragged last one at its
    own length."""
    n = len(x)
    w = oc.window_by_name(win, W) if win else np.ones(W, np.float32)
    n_chunks = -(-n // W)
    out = np.zeros(n_chunks * W, np.float32)
    for k in range(n_chunks):
        seg = x[k * W:(k + 1) * W]
        if k == 0:
            seg = np.concatenate([seg, np.zeros(W - len(seg), np.float32)])
        f = oc.toy_nnet(seg[None, None])[0, 0]
        out[k * W:k * W + len(f)] = f * w[:len(f)]
    return out[:n]


def _offline(mode, W, P, win, x):
    if mode == sr.OLA:
        return oc.overlap_add(oc.toy_nnet, x[None, None], W, P, win)[0, 0]
    if P == 0:
        return _boxcar_without_margin(x, W, win)
    return oc.overlap_add_boxcar(oc.toy_nnet, x[None, None], W, P, win)[0, 0]


def _model(mode, W, P, win, slots, defect=None, extra=37):
    need = W if mode == sr.OLA else W + 2 * P
    return sr.StreamModel(slots, mode, W, P, oc.window_by_name(win, W) if win else None,
                          np.float32(1.0 / (W / P)) if mode == sr.OLA else 1.0, need + extra, W + extra, defect=defect)


def _session(mode, W, P, win, seed, defect=None, max_rows=64, lengths=None, ops=None, after_feed=None, nnet=oc.toy_nnet, events=None):
    rng = np.random.default_rng(seed)
    lengths = _lengths(W) if lengths is None else lengths
    signals = [rng.uniform(-1, 1, n).astype(np.float32) for n in lengths]
    if events is None:
        events = sr.blocking(rng, lengths, sr.BLOCK_SIZES(W, P if mode == sr.OLA else max(P, 2)))
    m = _model(mode, W, P, win, len(lengths), defect)
    if ops is not None:
        ops.append("S %d %d %d %d %d %d" % (len(lengths), mode, W, P, m.cap_in, m.cap_out))
    return m, signals, sr.drive(m, nnet, signals, events, max_rows=max_rows, ops=ops, after_feed=after_feed)


@pytest.mark.parametrize("mode,W,P,win", CASES, ids=IDS)
def test_model_equals_the_offline_oracle_in_any_blocking(mode, W, P, win):
    tol = 2e-6 if mode == sr.OLA else 1e-6
    for seed in (1, 2):
        counts = []
        m, signals, outs = _session(mode, W, P, win, seed, max_rows=(64, 3)[seed - 1],
                                    after_feed=lambda s, fed, rel: counts.append((fed, rel)))
        assert counts
        for fed, rel in counts:     # the released counts, after every feed
            assert rel == sr.released_before_close(mode, W, P, fed), (fed, rel)
        for s, (x, y) in enumerate(zip(signals, outs)):
            ref = _offline(mode, W, P, win, x)
            assert y.shape == ref.shape and y.dtype == np.float32
            assert np.abs(y - ref).max() <= tol, (seed, len(x), np.abs(y - ref).max())
            assert m.state(s) == (len(x), len(x))      # after close: everything


def test_released_formulas_are_the_chunk_schedule():
    """The two formulas, from the definitions: a sample is final once the last chunk that holds it is stitched."""
    for W, H in OLA_SHAPES:
        for n in range(0, 4 * W):
            due = n // H                                   # chunks 1 .. n // H have run
            final = [t for t in range(n) if (t + W) // H <= due]
            assert sr.released_before_close(sr.OLA, W, H, n) == len(final), (W, H, n)
    for W, M in BOX_SHAPES:
        for n in range(0, 4 * W):
            frames = 0 if n < W + M else (n - M) // W       # frame k is due at (k + 1) W + M
            assert sr.released_before_close(sr.BOXCAR, W, M, n) == frames * W


def test_idle_and_empty_slots():
    """A slot that is closed after being fed nothing runs nothing and releases nothing; it does not disturb its neighbour."""
    m = _model(sr.OLA, 64, 16, "hanning", 2)
    a, b = m.open(), m.open()
    x = np.random.default_rng(3).uniform(-1, 1, 100).astype(np.float32)
    out = []
    for i in range(0, 100, 50):
        m.push([(a, x[i:i + 50]), (b, x[:0])])
        while len(c := m.next(8)):
            assert all(row.startswith("%d:" % a) for row in m.log[-1].split()[2:])     # never a row of the idle slot
            m.put(oc.toy_nnet(c[:, None])[:, 0])
        out += m.pop([a])
    m.close(b)
    assert m.st[b]["state"] == "closed" and m.state(b) == (0, 0)
    assert len(m.next(8)) == 0
    m.close(a)
    while len(c := m.next(8)):
        m.put(oc.toy_nnet(c[:, None])[:, 0])
    out += m.pop([a])
    assert np.abs(np.concatenate(out) - _offline(sr.OLA, 64, 16, "hanning", x)).max() <= 2e-6


def test_refusals_of_the_model():
    m = _model(sr.BOXCAR, 64, 8, None, 1, extra=0)
    s = m.open()
    with pytest.raises(sr.Refused):
        m.open()
    with pytest.raises(sr.Refused, match="overrun of slot 0"):
        m.push([(s, np.zeros(81, np.float32))])
    assert m.state(s) == (0, 0)
    with pytest.raises(sr.Refused):
        m.put(np.zeros((1, 72), np.float32))
    m.close(s)
    with pytest.raises(sr.Refused, match="not open"):
        m.push([(s, np.zeros(1, np.float32))])


# ---------------------------------------------------------------------------------------------------------------------------------
# planted defects: each one moves a sample's bits or the counts
# ---------------------------------------------------------------------------------------------------------------------------------
def _lookahead_net(x):
    """toy_nnet mirrored in time: every output sample depends on the NEXT input sample.  (toy_nnet is causal, so what a chunk holds
    past the end of its stream never reaches a sample that is kept.)"""
    return oc.toy_nnet(x[..., ::-1])[..., ::-1]


def _differs(mode, W, P, win, defect, **kw):
    _, _, good = _session(mode, W, P, win, 5, **kw)
    _, _, bad = _session(mode, W, P, win, 5, defect=defect, **kw)
    return any(g.shape != b.shape or not np.array_equal(g.view(np.uint32), b.view(np.uint32)) for g, b in zip(good, bad))


def test_planted_descending_accumulation_is_seen():
    assert _differs(sr.OLA, 64, 16, "hanning", "descending")      # H = W / 4: four terms per sample


def test_planted_missing_zero_fill_is_seen():
    assert _differs(sr.OLA, 64, 16, "hanning", "no_fill", nnet=_lookahead_net)
    # boxcar: the kept samples of a frame that reaches past the end lie a margin or more before it, except in a stream shorter than
    # one frame -- and there the ring holds something only when the slot has carried a stream before
    rng = np.random.default_rng(7)
    x0, x1 = (rng.uniform(-1, 1, n).astype(np.float32) for n in (150, 5))
    tails = []
    for defect in (None, "no_fill"):
        m = _model(sr.BOXCAR, 64, 8, None, 1, defect)
        tails.append([sr.drive(m, _lookahead_net, [x], [{0: len(x)}])[0] for x in (x0, x1)][1])
    assert tails[0].shape == tails[1].shape == (5,) and not np.array_equal(tails[0].view(np.uint32), tails[1].view(np.uint32))
    assert not _differs(sr.OLA, 64, 16, "hanning", "no_fill")      # ... and a causal network hides it: the GPU tests use both


def test_planted_late_wrap_is_seen():
    assert _differs(sr.OLA, 126, 21, None, "wrap")
    assert _differs(sr.BOXCAR, 126, 7, "hanning", "wrap")


def test_planted_back_margin_on_the_last_frame_is_seen():
    assert _differs(sr.BOXCAR, 64, 8, None, "back_margin")
    assert _differs(sr.BOXCAR, 126, 7, "hanning", "back_margin")


def test_planted_stale_accumulator_on_reuse_is_seen():
    """A slot is closed, opened again and fed another signal: with the accumulator left as the first stream's flush wrote it, the
    second stream's first samples carry its residue."""
    rng = np.random.default_rng(6)
    x0, x1 = (rng.uniform(-1, 1, n).astype(np.float32) for n in (150, 200))
    res = {}
    for defect in (None, "no_clear"):
        m = _model(sr.OLA, 64, 16, None, 1, defect)
        outs = [sr.drive(m, oc.toy_nnet, [x], [{0: len(x)}])[0] for x in (x0, x1)]
        assert m.log.count("open 0") == 2
        res[defect] = outs
    assert np.array_equal(res[None][0], res["no_clear"][0])
    assert np.abs(res[None][1] - _offline(sr.OLA, 64, 16, None, x1)).max() <= 2e-6
    assert not np.array_equal(res[None][1].view(np.uint32), res["no_clear"][1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's scheduler, as a sanitized stand-alone program, against the model's schedule
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sched_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the scheduler driver with")
    exe = str(tmp_path_factory.mktemp("stream_sched") / "stream_sched_main")
    # the sanitizer runtimes are linked into the program: it needs nothing preloaded and does not care what else is
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           *static, "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "stream_sched_main.cpp"),
           os.path.join(CSRC, "stream_sched.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _replay(exe, ops, tmp_path, name):
    path = tmp_path / (name + ".ops")
    path.write_text("\n".join(ops) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("mode,W,P,win", [c for c in CASES if c[3] is None], ids=[i for i, c in zip(IDS, CASES) if c[3] is None])
def test_scheduler_under_sanitizers_prints_the_models_schedule(sched_program, tmp_path, mode, W, P, win):
    # seeded blockings, and three streams fed in step (their chunks fall due together: groups of several rows, cut at max_rows)
    in_step = dict(lengths=[300, 300, 300], events=[{0: 50, 1: 50, 2: 50}] * 6)
    for seed, max_rows, kw in ((1, 64, {}), (2, 3, {}), (3, 1, {}), (4, 64, in_step), (5, 2, in_step)):
        ops = []
        m, _, _ = _session(mode, W, P, win, seed, max_rows=max_rows, ops=ops, **kw)
        got = _replay(sched_program, ops, tmp_path, "s%d" % seed)
        assert len(got) == len(m.log) and len(got) > 30
        for i, (a, b) in enumerate(zip(got, m.log)):
            assert a == b, "line %d: scheduler %r, model %r" % (i, a, b)
        if kw:
            most = max(line.count(" ") for line in got if line.startswith("next"))
            assert most - 1 >= 3 if max_rows == 64 else most - 1 == 2, most      # rows of the largest group


def test_scheduler_refusals_and_back_pressure(sched_program, tmp_path):
    """Refused calls change nothing; with a full output ring nothing more is scheduled until a pop makes room."""
    ops = ["S 2 0 64 16 64 64", "O", "P 1 0 65", "R 0", "P 1 1 1", "N 4", "C 1", "P 2 0 3 0 3",
           "P 1 0 64", "N 64", "R 0", "P 1 0 64", "N 64", "R 0", "N 64", "G 1 0", "N 64", "R 0", "C 0", "P 1 0 1", "O", "O"]
    got = _replay(sched_program, ops, tmp_path, "refusals")
    assert got[:8] == ["open 0", "push refused", "state 0 0 0 0 64", "push refused", "next 0", "close refused 1", "push refused",
                       "push 0:0:64:0"]
    # 64 samples: chunks 1..4 are due and release (4 + 1) * 16 - 64 = 16 samples
    assert got[8].startswith("next 64 0:-48:64:16 0:-32:64:32 0:-16:64:48 0:0:64:0") and got[9] == "put 0:0:4:1:0:64:16:16"
    assert got[10] == "state 0 64 16 16 16"
    # 64 more would overrun (room 16) -- refused; nothing is due
    assert got[11:14] == ["push refused", "next 0", "state 0 64 16 16 16"]
    assert got[14] == "next 0" and got[15] == "pop 0:0:16:0" and got[16] == "next 0"
    assert got[17] == "state 0 64 16 0 16"
    # slot 0 still has its flush to run, slot 1 was never opened: one more stream fits, a second does not
    assert got[18:] == ["close 0", "push refused", "open 1", "open refused"]


def test_scheduler_holds_chunks_back_while_the_output_ring_is_full(sched_program, tmp_path):
    ops = ["S 1 1 64 0 256 64", "O", "P 1 0 200", "N 8", "R 0", "N 8", "G 1 0", "N 8", "R 0", "G 1 0", "N 8", "R 0"]
    got = _replay(sched_program, ops, tmp_path, "pressure")
    assert got[1] == "push 0:0:200:0"
    assert got[2] == "next 64 0:0:200:0" and got[3] == "put 0:0:0:64:0"        # one frame fills the output ring of 64
    assert got[4] == "state 0 200 64 64 120" and got[5] == "next 0"             # frames 1 and 2 are due but held back
    assert got[6] == "pop 0:0:64:0"
    assert got[7] == "next 64 0:64:200:64" and got[8] == "put 0:0:0:64:64"
    assert got[9] == "state 0 200 128 64 184"
    assert got[10] == "pop 0:0:64:0" and got[11] == "next 64 0:128:200:128" and got[13] == "state 0 200 192 64 248"
