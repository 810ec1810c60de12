"""GPU: the silence and activity functions on the device (csrc/activity.hip: k_window_peaks, k_activity_decide) -- vfx_trim_bounds,
vfx_long_empty and vfx_active_frames against the host forms of voicefixer_main_amd.activity, which tests/test_activity_host.py holds
to the reference's own results and walks.  Everything compared is an integer: every bound, flag and label must be EQUAL.

Shapes at 44.1 kHz (segments of 882 samples, frames of 882 every 441), float32 and float64; the clips are those of
tests/activity_cases.py: zeros with ONE sample of twice the threshold at a window's last index, at the next window's first, at 0, 1,
441, n - 2 and n - 1; seeded speech-like clips; silent clips; and the golden's clips with the golden's parameters.  By the host forms
alone at most a quarter of them return None from trim_empty and every None case occurs (asserted below, and on the CPU in
test_activity_host.py, where the planted defects are shown to change a result on these clips)."""
import ctypes

import numpy as np
import pytest
import torch

import activity_cases as cases
from voicefixer_main_amd import activity

pytestmark = pytest.mark.gpu

DTYPES = {"float32": (np.float32, torch.float32), "float64": (np.float64, torch.float64)}
WHICH = ("tail", "head", "both")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voicefixer_main_amd.engine import Engine
    return Engine("cuda:0", config={"precision": 1})


@pytest.fixture(scope="module")
def clips():
    return {name: cases.planted_clips(nd) + cases.random_clips(nd) + cases.silent_clips(nd) for name, (nd, _) in DTYPES.items()}


def host_results(x, thr, sr=44100, fl=0.02, fs=0.01, long=None):
    """(tail, head, both, flag, labels or None) of one clip by the host forms"""
    long = cases.LONG if long is None else long
    return tuple(activity.trim_bounds(x, thr, sr, fl, w) for w in WHICH) + (
        activity.has_long_empty(x, threshold=thr, **long),
        activity.get_all_active_segment_index(x, thr, sr, fl, fs) if x.shape[0] > int(fs * sr) else None)


def _batch(rows, ld, fill, dtype):
    x = torch.full((len(rows), ld), fill, dtype=dtype)
    for b, c in enumerate(rows):
        x[b, :len(c)] = torch.from_numpy(c)
    return x


def device_results(eng, rows, thr, sr=44100, fl=0.02, fs=0.01, long=None, fill=0.0, extra=0, max_batch=128):
    """The same tuples from Engine.trim_bounds / has_long_empty / active_frames on padded batches of the clips in the given order"""
    long = cases.LONG if long is None else long
    out = []
    for a in range(0, len(rows), max_batch):
        part = rows[a:a + max_batch]
        lens = [len(c) for c in part]
        x = _batch(part, max(max(lens) + extra, 1), fill, torch.from_numpy(part[0]).dtype).to(eng.device)
        cols = []
        for w in WHICH:
            s, e = eng.trim_bounds(x, lens, thr, sr, fl, w)
            cols.append([None if i < 0 else (i, j) for i, j in zip(s.cpu().tolist(), e.cpu().tolist())])
            assert all((i < 0) == (j < 0) for i, j in zip(s.cpu().tolist(), e.cpu().tolist()))
        cols.append([bool(f) for f in eng.has_long_empty(x, lens, threshold=thr, **long).cpu().tolist()])
        labels = [None] * len(part)
        can = [b for b, n in enumerate(lens) if n > int(fs * sr)]
        if can:
            lab, cnt = eng.active_frames(x[can], [lens[b] for b in can], thr, sr, fl, fs)
            lab, cnt = lab.cpu().numpy(), cnt.cpu().tolist()
            for r, b in enumerate(can):
                assert cnt[r] == activity.active_frames_count(lens[b], sr, fl, fs) == eng.active_frames_count(lens[b], sr, fl, fs)
                assert not lab[r, cnt[r]:].any()
                labels[b] = lab[r, :cnt[r]].astype(int).tolist()
        cols.append(labels)
        out += list(zip(*cols))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs stay informative (CPU side)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_inputs_stay_informative(clips):
    g = cases.golden()
    thr, sr, fl = g["trims"][0]
    kinds = {}
    compared = [(x, cases.THR) for rows in clips.values() for x in rows] + [(g["x%d" % i], thr) for i in range(len(g["lengths"]))]
    for x, t in compared:
        k = cases.none_case(x, t)
        assert (k == "") == (activity.trim_bounds(x, t) is not None)
        kinds[k] = kinds.get(k, 0) + 1
    print(len(compared), kinds)
    assert set(kinds) == {"", "short", "one_segment", "silent", "dropped"}
    assert 4 * (len(compared) - kinds[""]) <= len(compared), kinds
    lens = {len(x) for x, _ in compared}
    assert set(cases.LENGTHS) <= lens and max(lens) == 65 * 1024 + 7 < 70000


# ---------------------------------------------------------------------------------------------------------------------------------
# every bound, flag and label equals the host form
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_planted_random_and_silent_clips_equal_the_host_forms(eng, clips, dtype):
    rows = clips[dtype]
    got = device_results(eng, rows, cases.THR)
    for i, x in enumerate(rows):
        assert got[i] == host_results(x, cases.THR), (i, len(x), int(np.flatnonzero(x)[0]) if x.any() else None)
    assert sum(r[3] for r in got) > 10 and sum(not r[3] for r in got) > 10
    assert sum(1 for r in got if r[4] and any(r[4]) and not all(r[4])) > 100


def test_golden_clips_with_the_goldens_parameters(eng):
    g = cases.golden()
    rows = [g["x%d" % i] for i in range(len(g["lengths"]))]
    for dt in (np.float32, np.float64):
        part = [x for x in rows if x.dtype == dt]
        ids = [i for i, x in enumerate(rows) if x.dtype == dt]
        for p, (thr, sr, fl) in enumerate(g["trims"]):
            q = min(p, 1)
            fthr, fsr, ffl, ffs = g["frames"][q]
            length, lsr = g["longs"][q]
            long = dict(length=float(length), sample_rate=int(lsr))
            got = device_results(eng, part, float(thr), int(sr), float(fl), float(ffs), long)
            for i, x, r in zip(ids, part, got):
                want = [None if b[0] < 0 else (int(b[0]), int(b[1])) for b in g["bounds%d" % i][p]]
                assert list(r[:3]) == want == list(host_results(x, float(thr), int(sr), float(fl), float(ffs), long)[:3]), (i, p)
            # the flags at the reference's own 400 and the labels at the golden's frame parameters
            for i, x in zip(ids, part):
                if len(x):
                    flag = eng.has_long_empty(torch.from_numpy(x), None, float(length), int(lsr), 400)
                    assert bool(flag[0]) is bool(g["long%d" % i][q]), (i, q)
                key = "labels%d_%d" % (i, q)
                if key in g:
                    lab, cnt = eng.active_frames(torch.from_numpy(x), None, float(fthr), int(fsr), float(ffl), float(ffs))
                    assert lab[0, :int(cnt[0])].cpu().tolist() == g[key].tolist(), (i, q)


# ---------------------------------------------------------------------------------------------------------------------------------
# a clip's results do not depend on the batch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_padded_batch_equals_single_calls(eng, clips, dtype):
    rows = clips[dtype]
    n_planted = len(cases.planted_clips(DTYPES[dtype][0]))
    by_len = {}
    for i, x in enumerate(rows[:n_planted]):
        by_len.setdefault(len(x), []).append(i)
    pick = [ids[len(ids) // 2] for ids in by_len.values()] + [ids[-1] for ids in by_len.values()]
    pick += list(range(n_planted, n_planted + 12))                 # the first random clips have the lengths of LENGTHS
    some = [rows[i] for i in pick]
    singles = device_results(eng, some, cases.THR, max_batch=1)
    assert singles == [host_results(x, cases.THR) for x in some]
    longest = max(len(x) for x in some)
    for fill in (1e30, float("nan")):
        # an odd row stride (misaligned rows) and a 16-byte-aligned one, both with samples past the longest clip's end
        for ld in ((longest + 2) | 1, (longest + 8) // 4 * 4):
            extra = ld - longest
            assert extra >= 2 and (ld % 2 == 1 or ld % 4 == 0)
            for order in (list(range(len(some))), list(range(len(some)))[::-1]):
                got = device_results(eng, [some[j] for j in order], cases.THR, fill=fill, extra=extra)
                assert got == [singles[j] for j in order], (fill, extra)


def test_130_clips_cross_the_sub_batch(eng):
    rows = cases.random_clips(np.float32, count=130, seed=11)
    lens = [len(x) for x in rows]
    x = _batch(rows, max(lens) + 3, float("nan"), torch.float32).to(eng.device)
    s, e = eng.trim_bounds(x, lens, cases.THR)
    flag = eng.has_long_empty(x, lens, threshold=cases.THR, **cases.LONG)
    lab, cnt = eng.active_frames(x, lens, cases.THR)
    s, e, flag, lab, cnt = s.cpu().tolist(), e.cpu().tolist(), flag.cpu().tolist(), lab.cpu().numpy(), cnt.cpu().tolist()
    for i, c in enumerate(rows):
        want = host_results(c, cases.THR)
        assert (None if s[i] < 0 else (s[i], e[i])) == want[2] and bool(flag[i]) is want[3] and lab[i, :cnt[i]].tolist() == want[4], i


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(eng):
    from voicefixer_main_amd.engine import _ptr
    B, L = 2, 3000
    x = torch.zeros(B, L, device=eng.device)
    start = torch.full((B,), -7, device=eng.device, dtype=torch.int64)
    stop, counts = start.clone(), start.clone()
    flag = torch.full((B,), -7, device=eng.device, dtype=torch.int32)
    labels = torch.full((B, 8), 9, device=eng.device, dtype=torch.uint8)
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)

    def trim(wav=x, b=B, ld=L, lens=(L, L), seg=882, thr=0.1, which=2, s=start, e=stop, f64=0):
        return eng.lib.vfx_trim_bounds(eng.h, _ptr(wav), f64, b, ld, None if lens is None else i64(lens), seg, thr, which, _ptr(s), _ptr(e),
                                       eng._stream())

    def long(wav=x, b=B, ld=L, lens=(L, L), seg=882, step=4410, thr=0.1, f=flag):
        return eng.lib.vfx_long_empty(eng.h, _ptr(wav), 0, b, ld, None if lens is None else i64(lens), seg, step, thr, _ptr(f), eng._stream())

    def frames(wav=x, b=B, ld=L, lens=(L, L), frame=882, shift=441, thr=0.1, lab=labels, ldf=8, cnt=counts):
        return eng.lib.vfx_active_frames(eng.h, _ptr(wav), 0, b, ld, None if lens is None else i64(lens), frame, shift, thr, _ptr(lab), ldf,
                                         _ptr(cnt), eng._stream())

    nan, inf = float("nan"), float("inf")
    cases_ = [(trim, dict(wav=None), "vfx_trim_bounds: NULL"), (trim, dict(lens=None), "NULL"), (trim, dict(s=None), "NULL"),
              (trim, dict(e=None), "NULL"), (trim, dict(b=0), "0 clips (need 1 <= B <= 1024)"), (trim, dict(b=1025), "1025 clips"),
              (trim, dict(lens=(L, L + 1)), "vfx_trim_bounds: clip 1 has 3001 samples, the rows hold 3000"),
              (trim, dict(lens=(-1, L)), "clip 0 has a negative length"), (trim, dict(seg=0), "seg = 0"), (trim, dict(seg=-5), "seg = -5"),
              (trim, dict(thr=nan), "threshold = nan"), (trim, dict(thr=inf), "threshold = inf"), (trim, dict(which=3), "which = 3"),
              (trim, dict(f64=2), "x_f64 = 2"),
              (long, dict(wav=None), "vfx_long_empty: NULL"), (long, dict(f=None), "NULL"), (long, dict(b=0), "0 clips"),
              (long, dict(lens=(L + 1, L)), "vfx_long_empty: clip 0 has 3001 samples"), (long, dict(seg=0), "seg = 0"),
              (long, dict(step=0), "step = 0"), (long, dict(thr=-inf), "threshold = -inf"),
              (frames, dict(wav=None), "vfx_active_frames: NULL"), (frames, dict(lab=None), "NULL"), (frames, dict(b=1025), "1025 clips"),
              (frames, dict(lens=(L, 441)), "vfx_active_frames: clip 1 has 441 samples: the length must be greater than the reflect "
                                            "padding, which is 441"),
              (frames, dict(lens=(L, 0)), "clip 1 has 0 samples"), (frames, dict(lens=(L + 1, L)), "clip 0 has 3001 samples"),
              (frames, dict(frame=0), "frame = 0"), (frames, dict(shift=0), "shift = 0"), (frames, dict(thr=nan), "threshold = nan"),
              (frames, dict(ldf=6), "clip 0 has 7 frames, the label rows hold 6"), (frames, dict(ldf=0), "ldf = 0")]
    for fn, kw, text in cases_:
        assert fn(**kw) != 0, kw
        assert text in eng.lib.vfx_last_error().decode(), (kw, eng.lib.vfx_last_error())
    torch.cuda.synchronize()
    for t in (start, stop, counts, flag):
        assert bool((t == -7).all())
    assert bool((labels == 9).all())
    # inside the ranges: lengths 0 for the trims and the flag, counts = NULL, a length of shift + 1, a threshold of 0
    assert trim(lens=(0, L), thr=0.0) == 0 and long(lens=(0, L)) == 0 and frames(lens=(442, L), cnt=None) == 0
    torch.cuda.synchronize()
    # (against a threshold of 0 nothing is quiet: the zeros are kept whole)
    assert start.tolist() == [-1, 0] and stop.tolist() == [-1, L] and flag.tolist() == [0, 1]
    assert labels.tolist() == [[0] * 8, [0] * 8] and bool((counts == -7).all())
    with pytest.raises(RuntimeError, match="clip 0 has 441 samples"):
        eng.active_frames(torch.zeros(441))
    with pytest.raises(ValueError, match="3 lengths for 2 clips"):
        eng.trim_bounds(x, lengths=[L, L, L])
    with pytest.raises(ValueError, match="float32 or float64"):
        eng.trim_bounds(torch.zeros(3000, dtype=torch.int16))
    with pytest.raises(ValueError, match="which"):
        eng.trim_bounds(x, which="middle")


# ---------------------------------------------------------------------------------------------------------------------------------
# list forms, device-resident
# ---------------------------------------------------------------------------------------------------------------------------------
def test_list_forms_on_the_device_equal_the_host_forms(eng, clips):
    f32, f64 = clips["float32"], clips["float64"]
    n_planted = len(cases.planted_clips(np.float32))
    pcm = (cases.speechlike(5000, 77, np.float64) * 2 ** 15).astype(np.int16)       # another dtype: the host form
    some = f32[5:n_planted:9] + f64[n_planted:n_planted + 20] + [torch.from_numpy(c).to(eng.device) for c in f32[n_planted + 20:n_planted + 30]]
    some += [np.zeros(0, np.float32), np.zeros(300, np.float64), f32[-2], f64[-1]]
    as_np = [c.cpu().numpy() if isinstance(c, torch.Tensor) else c for c in some]
    thr = cases.THR
    for fn, hostfn in ((activity.trim_tail_empty_list, activity.trim_tail_empty), (activity.trim_head_empty_list, activity.trim_head_empty),
                       (activity.trim_empty_list, activity.trim_empty)):
        got = fn(some, thr, engine=eng, to_host=False)
        for c, y in zip(as_np, got):
            want = hostfn(c, thr)
            assert (y is None) == (want is None)
            if want is not None:
                assert isinstance(y, torch.Tensor) and y.device == eng.device and y.dtype == torch.from_numpy(c).dtype
                assert np.array_equal(y.cpu().numpy(), want)
    assert sum(y is None for y in got) >= 3 and sum(y is not None for y in got) >= 20
    assert activity.trim_empty_bounds_list(some, thr, engine=eng) == [activity.trim_bounds(c, thr) for c in as_np]
    back = activity.trim_empty_list(some, thr, engine=eng)
    assert all(y is None or isinstance(y, np.ndarray) for y in back)
    assert all((y is None and w is None) or np.array_equal(y, w) for y, w in zip(back, [activity.trim_empty(c, thr) for c in as_np]))
    # PCM integers take the host form, at the reference's own threshold
    mixed = [pcm, f32[n_planted + 3]]
    assert activity.trim_empty_bounds_list(mixed, 500, engine=eng) == [activity.trim_bounds(pcm, 500), activity.trim_bounds(mixed[1], 500)]
    flags = activity.has_long_empty_list(some, threshold=thr, engine=eng, to_host=False, **cases.LONG)
    want = [activity.has_long_empty(c, threshold=thr, **cases.LONG) for c in as_np]
    assert flags.device == eng.device and flags.dtype == torch.bool and flags.cpu().tolist() == want and 0 < sum(want) < len(want)
    assert activity.has_long_empty_list(some, threshold=thr, engine=eng, **cases.LONG) == want
    nonempty = [c for c in some if c.shape[0]]
    labels = activity.active_frames_list(nonempty, thr, engine=eng, to_host=False)
    for c, y in zip(nonempty, labels):
        c = c.cpu().numpy() if isinstance(c, torch.Tensor) else c
        assert y.device == eng.device and y.dtype == torch.uint8 and y.cpu().tolist() == activity.get_all_active_segment_index(c, thr)
    assert activity.active_frames_list(nonempty[:5], thr, engine=eng) == [y.cpu().tolist() for y in labels[:5]]
    # max_mag_unify_list: est scaled to ref's peak, one multiplication per sample in the clip's dtype
    refs = f32[n_planted:n_planted + 6] + f64[n_planted:n_planted + 6] + [f64[n_planted + 7], pcm]
    ests = f32[n_planted + 6:n_planted + 12] + f64[n_planted + 6:n_planted + 12] + [f32[n_planted + 8], pcm[:400]]
    r, got = activity.max_mag_unify_list(refs, ests, engine=eng, to_host=False)
    assert r is not None and all(a is b for a, b in zip(r, refs))
    for a, b, y in zip(refs, ests, got):
        want = activity.max_mag_unify(a, b)[1]
        assert y.device == eng.device and y.dtype == torch.from_numpy(want).dtype and np.array_equal(y.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# restore_trimmed_list
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["voicefixer", "ssr_unet"])
def test_restore_trimmed_list_restores_the_active_spans_only(kind):
    from voicefixer_main_amd import models, synth
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_MEL, MODEL_UNET_SPEC, MODEL_VOCODER
    e = Engine("cuda:0", config={"precision": 1})
    if kind == "voicefixer":
        e.load_state_dict(MODEL_UNET_MEL, synth.make_resunet_state_dict(0))
        e.load_state_dict(MODEL_VOCODER, synth.make_vocoder_state_dict(1))
        model = models.VoiceFixer(engine=e)
    else:
        e.load_state_dict(MODEL_UNET_SPEC, synth.make_resunet_state_dict(2))
        model = models.SSR_UNet(engine=e)
    mid = np.zeros(9001, np.float32)
    mid[3000:6000] = 0.1 * np.random.default_rng(0).standard_normal(3000)
    short = np.zeros(100 + 3 * 882, np.float32)
    short[:1800] = 0.1 * np.random.default_rng(1).standard_normal(1800)       # trim_empty keeps (0, 982): widened to (0, 1025)
    wavs = [mid, np.zeros(4000, np.float32), short, cases.speechlike(7000, 6, np.float32), np.zeros(881, np.float32)]
    wavs = [torch.from_numpy(w) for w in wavs]
    found = [activity.trim_bounds(w.numpy(), cases.THR) for w in wavs]
    assert found[0] == (1764, 5473) and found[1] is None and found[2] == (0, 982) and found[3] is not None and found[4] is None
    outs, bounds = model.restore_trimmed_list(wavs)
    assert bounds == [found[0], None, (0, 1025), found[3], None]
    keep = [i for i, b in enumerate(bounds) if b is not None]
    want = model.restore_list([wavs[i][bounds[i][0]:bounds[i][1]] for i in keep])
    for i, y in zip(keep, want):
        s, t = bounds[i]
        assert outs[i].shape == wavs[i].shape and torch.equal(outs[i][s:t], y) and bool(y.any()), i
        assert not outs[i][:s].any() and not outs[i][t:].any()
        assert torch.equal(y, model.restore_list([wavs[i][s:t]])[0])           # ... which is that span's own call
    for i in (1, 4):
        assert outs[i].shape == wavs[i].shape and not outs[i].any()
    # an all-silent list launches nothing of the network: no tap-convolution launch is recorded
    e.profile_begin()
    outs, bounds = model.restore_trimmed_list([torch.zeros(4000), torch.zeros(881), torch.zeros(2 * 882)])
    assert e.profile_end()[0] == 0
    assert bounds == [None, None, None] and [tuple(o.shape) for o in outs] == [(4000,), (881,), (1764,)] and not any(o.any() for o in outs)
    e.profile_begin()
    model.restore_trimmed_list([wavs[0]])
    assert e.profile_end()[0] > 0
    e.close()
