"""CPU: the host forms of voicefixer_main_amd.activity -- the closed forms over window peaks that csrc/activity.hip evaluates --
against the reference's own results (tests/golden/activity.npz, scripts/gen_golden_activity.py) and against the reference's walks
restated (tests/activity_cases.py) on random small clips; the None cases, the strictness of the two comparisons, NaN samples, the
threshold's rounding to the clip's dtype; the defects the GPU tests' clips must be able to see; the list layer of
restore_trimmed_list against a recording model; the C ABI's declaration."""
import os
import re
import types

import numpy as np
import pytest
import torch

import activity_cases as cases
from voicefixer_main_amd import activity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bounds(b):
    return None if b[0] < 0 else (int(b[0]), int(b[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's results
# ---------------------------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_reference_exactly():
    g = cases.golden()
    assert os.path.getsize(cases.GOLDEN) < 100 << 10
    some_none = some_kept = some_cut = 0
    for i, n in enumerate(g["lengths"]):
        x = g["x%d" % i]
        assert x.shape == (n,) and x.dtype in (np.float32, np.float64)
        for p, (thr, sr, fl) in enumerate(g["trims"]):
            sr = int(sr)
            want = [_bounds(b) for b in g["bounds%d" % i][p]]
            for which, w, fn in zip(("tail", "head", "both"), want, (activity.trim_tail_empty, activity.trim_head_empty, activity.trim_empty)):
                assert activity.trim_bounds(x, thr, sr, fl, which) == w, (i, p, which)
                y = fn(x, threshold=thr, sample_rate=sr, frame_length=fl)
                if w is None:
                    assert y is None
                    some_none += 1
                else:
                    assert np.shares_memory(y, x) or y.size == 0
                    assert np.array_equal(y, x[w[0]:w[1]]) and y.shape[0] == w[1] - w[0]
                    some_kept += w == (0, n)
                    some_cut += w != (0, n)
        for p, (length, sr) in enumerate(g["longs"]):
            assert activity.has_long_empty(x, length=length, sample_rate=int(sr)) is bool(g["long%d" % i][p]), (i, p)
        for p, (thr, sr, fl, fs) in enumerate(g["frames"]):
            key = "labels%d_%d" % (i, p)
            if key in g:
                got = activity.get_all_active_segment_index(x, thr, int(sr), fl, fs)
                assert isinstance(got, list) and got == g[key].tolist(), (i, p)
                assert len(got) == activity.active_frames_count(n, int(sr), fl, fs)
        if n:
            assert [int(activity.is_valid_signal(x, threshold=t)) for t in (1000, 2999, 3000)] == g["valid%d" % i].tolist()
    assert some_none > 10 and some_kept > 10 and some_cut > 10
    for j, (a, b) in enumerate(g["unify_pairs"]):
        ref, est = g["x%d" % a], g["x%d" % b]
        r, e = activity.max_mag_unify(ref, est)
        assert r is ref and e.dtype == g["unify%d" % j].dtype and np.array_equal(e, g["unify%d" % j])
    assert activity.trim_empty(None) is None and activity.trim_tail_empty(None) is None and activity.has_long_empty(None) is None
    # the defaults are the reference's
    x = g["x10"]
    assert np.array_equal(activity.trim_empty(x), activity.trim_empty(x, 500, 44100, 0.02))
    assert activity.get_all_active_segment_index(x) == activity.get_all_active_segment_index(x, 500, 44100, 0.02, 0.01)
    assert activity.has_long_empty(np.zeros(3 * 44100 + 1)) is True and activity.has_long_empty(np.zeros(3 * 44100)) is False
    assert activity.has_long_empty(np.full(3 * 44100 + 1, 400.0)) is False


# ---------------------------------------------------------------------------------------------------------------------------------
# closed forms against the walks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_closed_forms_equal_the_walks_on_random_small_clips(dtype):
    rng = np.random.default_rng(0)
    seg, none, total = 8, 0, 4000
    for _ in range(total):
        n = int(rng.integers(0, 71))
        w = np.zeros(n, dtype)
        if n and rng.random() < 0.9:
            a = int(rng.integers(0, n))
            b = int(rng.integers(a, n + 1))
            w[a:b] = rng.uniform(-2, 2, b - a)
        if n and rng.random() < 0.3:
            w[int(rng.integers(0, n))] = rng.uniform(-2, 2)
        peak, thr = cases.row_peak(w, n), dtype(1.0)
        want = (cases.walk_tail(n, seg, thr, peak), cases.walk_head(n, seg, thr, peak), cases.walk_both(n, seg, thr, peak))
        got = tuple(activity.trim_bounds(w, 1.0, 400, 0.02, which) for which in ("tail", "head", "both"))
        assert got == want, (w.tolist(), got, want)
        assert activity.has_long_empty(w, length=2, sample_rate=4, threshold=1.0) == cases.walk_long(n, 8, 4, thr, peak)
        if n > 4:
            assert activity.get_all_active_segment_index(w, 1.0, 400, 0.02, 0.01) == cases.walk_frames(w, n, 8, 4, thr)
        none += want[2] is None
    assert int(400 * 0.02) == 8 and int(0.01 * 400) == 4
    assert 0.2 < none / total < 0.8


def test_none_cases_and_kept_quirks():
    seg, thr = cases.SEG, cases.THR
    loud = lambda n, lo, hi: np.concatenate([np.zeros(lo, np.float32), np.full(hi - lo, 0.5, np.float32), np.zeros(n - hi, np.float32)])
    kw = dict(threshold=thr)
    # n < seg: None, whatever the clip holds; n == 0 too
    assert activity.trim_tail_empty(loud(seg - 1, 0, seg - 1), **kw) is None and activity.trim_empty(np.zeros(0, np.float32), **kw) is None
    # n == seg: the tail keeps it whole without a look, the head has no s < n - seg = 0
    for x in (loud(seg, 0, seg), np.zeros(seg, np.float32)):
        assert activity.trim_tail_empty(x, **kw).shape[0] == seg and activity.trim_head_empty(x, **kw) is None
        assert activity.trim_empty(x, **kw) is None
    # all silent: on the grid from n down to the window that ends at seg -> L == seg -> the EMPTY clip, which is not None; with a
    # remainder the walk ends at L = r < seg -> None
    assert activity.trim_tail_empty(np.zeros(4 * seg, np.float32), **kw).shape[0] == 0
    assert activity.trim_tail_empty(np.zeros(4 * seg + 5, np.float32), **kw) is None
    assert activity.trim_empty(np.zeros(4 * seg, np.float32), **kw) is None and activity.trim_head_empty(np.zeros(4 * seg), **kw) is None
    # active only in the segment the tail rule drops: once the tail has dropped a quiet segment it drops the next one as well
    x = loud(4 * seg, seg, 2 * seg)
    assert activity.trim_bounds(x, thr, which="tail") == (0, seg) and activity.trim_bounds(x, thr, which="head") == (0, 4 * seg)
    assert activity.trim_empty(x, **kw) is None
    # ... and the head keeps one quiet segment
    x = loud(6 * seg, 3 * seg, 6 * seg)
    assert activity.trim_bounds(x, thr) == (2 * seg, 6 * seg)
    for name, x in (("short", loud(seg - 1, 0, 5)), ("one_segment", loud(seg, 0, seg)), ("silent", np.zeros(3000, np.float32)),
                    ("dropped", loud(4 * seg, seg, 2 * seg)), ("", loud(6 * seg, 3 * seg, 6 * seg))):
        assert cases.none_case(x) == name
    with pytest.raises(ValueError):
        activity.trim_empty(x, sample_rate=10)
    with pytest.raises(ValueError):
        activity.trim_bounds(x, which="middle")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_comparisons_are_strict_and_a_nan_is_neither(dtype):
    seg, t = cases.SEG, 0.25
    x = np.zeros(6 * seg, dtype)
    x[3 * seg + 5] = t                          # a peak EQUAL to the threshold is not quiet (<) and not valid (>)
    assert activity.trim_bounds(x, t, which="tail") == (0, 3 * seg) and activity.trim_bounds(x, t, which="head") == (2 * seg, 6 * seg)
    assert activity.trim_bounds(x, np.nextafter(dtype(t), dtype(1)), which="head") is None
    assert not any(activity.get_all_active_segment_index(x, t)) and not activity.is_valid_signal(x, t)
    assert sum(activity.get_all_active_segment_index(x, np.nextafter(dtype(t), dtype(0)))) == 2
    y = np.full(3 * seg, t, dtype)
    assert activity.has_long_empty(y, length=0.02, threshold=t) is False
    assert activity.has_long_empty(y, length=0.02, threshold=np.nextafter(dtype(t), dtype(1))) is True
    x[3 * seg + 5] = np.nan                     # a NaN peak: not < threshold -> active for the trims; not > threshold -> label 0
    assert activity.trim_bounds(x, t, which="tail") == (0, 3 * seg) and activity.trim_bounds(x, t, which="head") == (2 * seg, 6 * seg)
    assert not any(activity.get_all_active_segment_index(x, t)) and not activity.is_valid_signal(x, t)
    z = np.zeros(3 * seg, dtype)
    z[seg + 1] = np.nan
    assert activity.has_long_empty(z, length=0.02, threshold=t) is True       # (the other windows are quiet)
    z[:] = np.nan
    assert activity.has_long_empty(z, length=0.02, threshold=t) is False


def test_threshold_is_rounded_to_the_clips_dtype():
    t = 0.7                                     # float32(0.7) < 0.7, float32(0.1) > 0.1
    assert float(np.float32(t)) < t
    seg = cases.SEG
    x = np.zeros(6 * seg, np.float32)
    x[3 * seg] = np.float32(t)                  # in float64 this peak is below t; compared in float32 it EQUALS the threshold
    assert activity.trim_bounds(x, t, which="head") == (2 * seg, 6 * seg)
    assert activity.trim_bounds(x.astype(np.float64), t, which="head") is None
    t = 0.1
    assert float(np.float32(t)) > t
    x[3 * seg] = np.float32(t)                  # in float64 this peak is above t; in float32 it is not
    assert not any(activity.get_all_active_segment_index(x, t)) and not activity.is_valid_signal(x, t)
    assert any(activity.get_all_active_segment_index(x.astype(np.float64), t))
    # PCM integers are left to NumPy's own promotion
    pcm = np.zeros(6 * seg, np.int16)
    pcm[3 * seg] = 500
    assert activity.trim_bounds(pcm, 500, which="head") == (2 * seg, 6 * seg) and activity.trim_bounds(pcm, 500.5, which="head") is None


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU tests' clips see the defects, and stay informative
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_clips():
    return {dt: cases.planted_clips(dt) + cases.random_clips(dt) + cases.silent_clips(dt) for dt in (np.float32, np.float64)}


def _row(x, fill):
    return np.concatenate([x, np.full(8, fill, x.dtype)])


@pytest.mark.parametrize("defect", cases.DEFECTS)
def test_planted_defects_change_a_result_on_the_gpu_clips(gpu_clips, defect):
    changed = {"planted": 0, "random": 0}
    clips = gpu_clips[np.float32]
    n_planted = len(cases.planted_clips(np.float32))
    for i, x in enumerate(clips[:n_planted + 40]):
        n = x.shape[0]
        good = cases.results(_row(x, 1e30), n, cases.THR)
        assert good == cases.results(_row(x, np.nan), n, cases.THR) == cases.results(x, n, cases.THR)      # nothing past the end counts
        bad = cases.results(_row(x, 1e30), n, cases.THR, defect)
        changed["planted" if i < n_planted else "random"] += bad != good
    print(defect, changed)
    assert changed["planted"] >= 2, changed


def test_host_forms_equal_the_walks_on_the_gpu_clips_and_the_clips_stay_informative(gpu_clips):
    for dt, clips in gpu_clips.items():
        kinds = {}
        for x in clips:
            n = x.shape[0]
            want = cases.results(x, n, cases.THR)
            got = (activity.trim_bounds(x, cases.THR, which="tail"), activity.trim_bounds(x, cases.THR, which="head"),
                   activity.trim_bounds(x, cases.THR), activity.has_long_empty(x, threshold=cases.THR, **cases.LONG),
                   activity.get_all_active_segment_index(x, cases.THR))
            assert got == want
            kinds[cases.none_case(x)] = kinds.get(cases.none_case(x), 0) + 1
        print(dt.__name__, kinds)
        assert set(kinds) == {"", "short", "one_segment", "silent", "dropped"}
        assert 4 * (len(clips) - kinds[""]) <= len(clips), kinds


# ---------------------------------------------------------------------------------------------------------------------------------
# restore_trimmed_list's list layer
# ---------------------------------------------------------------------------------------------------------------------------------
class _StubEngine:
    device = torch.device("cpu")
    cfg = types.SimpleNamespace(sample_rate=44100)

    def trim_bounds(self, x, lengths, threshold, sample_rate, frame_length, which):
        b = [activity.trim_bounds(x[j, :n].numpy(), threshold, sample_rate, frame_length, which) for j, n in enumerate(lengths)]
        return (torch.tensor([-1 if v is None else v[0] for v in b]), torch.tensor([-1 if v is None else v[1] for v in b]))


class _Recorder:
    def __init__(self):
        self.engine, self.calls = _StubEngine(), []

    def restore_list(self, wavs, **kwargs):
        self.calls.append(([w.clone() for w in wavs], kwargs))
        return [w + 1.0 for w in wavs]


def test_trimmed_span_widens_right_then_left():
    from voicefixer_main_amd.models import trimmed_span, MIN_RESTORE_SAMPLES
    assert MIN_RESTORE_SAMPLES == 1025
    assert trimmed_span((100, 5000), 6000) == (100, 5000)
    assert trimmed_span((100, 1125), 6000) == (100, 1125)
    assert trimmed_span((100, 1124), 6000) == (100, 1125)               # to the right
    assert trimmed_span((5500, 5900), 6000) == (4975, 6000)             # to the clip's end, then to the left
    assert trimmed_span((0, 982), 1025) == (0, 1025)
    assert trimmed_span((10, 900), 1000) == (0, 1000)                   # a clip below the minimum goes in whole


def test_restore_trimmed_list_with_a_recording_model():
    from voicefixer_main_amd import models
    seg, thr = cases.SEG, cases.THR
    n_short = 100 + 3 * seg
    short = np.zeros(n_short, np.float32)
    short[:1800] = 0.5                                                   # trim_empty keeps (0, 982): below the minimum
    mid = np.zeros(9001, np.float32)
    mid[3000:6000] = 0.5                                                 # (1764, 5473): a quiet segment kept in front, one dropped behind
    wavs = [mid, np.zeros(4000, np.float32), short, cases.speechlike(7000, 6, np.float64)]
    want = [activity.trim_bounds(w.astype(np.float32), thr) for w in wavs]
    assert want[1] is None and want[2] == (0, 982) and want[0] == (1764, 5473) and want[3] is not None
    model = _Recorder()
    outs, bounds = models._restore_trimmed_list(model, [torch.from_numpy(w) for w in wavs], thr, 0.02, {"max_batch": 7})
    assert bounds == [want[0], None, (0, 1025), want[3]]
    assert len(model.calls) == 1 and model.calls[0][1] == {"max_batch": 7} and len(model.calls[0][0]) == 3
    for i, sent in zip((0, 2, 3), model.calls[0][0]):
        s, e = bounds[i]
        x = torch.from_numpy(wavs[i].astype(np.float32))
        assert sent.dtype == torch.float32 and torch.equal(sent, x[s:e])
        assert outs[i].shape == x.shape and torch.equal(outs[i][s:e], x[s:e] + 1.0)
        assert not outs[i][:s].any() and not outs[i][e:].any()
    assert outs[1].shape == (4000,) and not outs[1].any()
    # only silent clips: no restore call at all
    model = _Recorder()
    outs, bounds = models._restore_trimmed_list(model, [torch.zeros(3000), torch.zeros(881)], thr, 0.02, {})
    assert model.calls == [] and bounds == [None, None] and [tuple(o.shape) for o in outs] == [(3000,), (881,)] and not any(o.any() for o in outs)
    for cls in (models.VoiceFixer, models.SSR_UNet):
        assert cls.restore_trimmed_list.__defaults__ == (500 / 2 ** 15, 0.02)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI and the Python surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_is_declared_and_bound():
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    for name, nargs in (("vfx_trim_bounds", 12), ("vfx_long_empty", 11), ("vfx_active_frames", 13), ("vfx_active_frames_count", 3)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, "%s is not declared in include/vfx.h" % name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
    assert re.search(r"VFX_TRIM_TAIL = 0, VFX_TRIM_HEAD = 1, VFX_TRIM_BOTH = 2", header)
    assert (_lib.TRIM_TAIL, _lib.TRIM_HEAD, _lib.TRIM_BOTH) == (0, 1, 2)
    for name in ("trim_bounds", "has_long_empty", "active_frames"):
        assert callable(getattr(Engine, name))
    src = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "activity.hip")).read()
    assert "k_window_peaks" in src and "k_activity_decide" in src and "clip_batch.h" in src
    assert "activity.hip" in open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "Makefile")).read()
    for name in ("trim_tail_empty_list", "trim_head_empty_list", "trim_empty_list", "trim_empty_bounds_list", "has_long_empty_list",
                 "active_frames_list", "max_mag_unify_list"):
        assert callable(getattr(activity, name))
    lib = _lib.load()
    assert lib.vfx_active_frames_count(44100, 882, 441) == 101 == activity.active_frames_count(44100)
    assert lib.vfx_active_frames_count(441, 882, 441) == 2 and lib.vfx_active_frames_count(10, 0, 441) == -1
