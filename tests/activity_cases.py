"""What tests/test_activity_host.py and tests/test_gpu_activity.py share: the reference's walks (tools/others/audio_op.py:79-147)
restated over a window-peak oracle, so that the defects a padded-batch kernel can have are planted in ONE place, and the clips of the
GPU tests, built on the CPU with a fixed seed.

The walks take `peak(lo, hi)` = max |x[lo:hi]| and return bounds, not arrays: (start, stop) or None.  `row_peak` is that oracle over
a padded ROW (the clip's first n samples, then whatever the batch holds), with the defects:

    "seam"      a window misses its last sample (an off-by-one seam between neighbouring windows)
    "past_end"  the group that holds the clip's last sample is read whole: up to three samples past the clip's end
    "anchor0"   (walk_tail) the tail's windows lie on the grid from 0, not on the grid that ends at n
    "edge"      (walk_frames) the padding repeats the edge sample (np.pad's "symmetric")
"""
import os

import numpy as np

SEG, FRAME, SHIFT = 882, 882, 441          # int(44100 * 0.02), int(0.02 * 44100), int(0.01 * 44100)
THR = 500 / 2 ** 15                        # the reference's default on the float scale
LONG = dict(length=0.2, sample_rate=4410)  # has_long_empty with windows of 882 samples every 4410
LENGTHS = (881, 882, 883, 1764, 1764 + 301, 9001, 65 * 1024 + 7)
DEFECTS = ("seam", "past_end", "anchor0", "edge")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activity.npz")


# ---------------------------------------------------------------------------------------------------------------------------------
# the walks
# ---------------------------------------------------------------------------------------------------------------------------------
def row_peak(row, n, defect=None):
    row = np.asarray(row)

    def peak(lo, hi):
        if defect == "seam":
            hi -= 1
        if defect == "past_end" and hi == n:
            hi = -(-n // 4) * 4
        return np.max(np.abs(row[lo:hi]))
    return peak


def walk_tail(n, seg, thr, peak, defect=None):
    top = n - n % seg if defect == "anchor0" else n
    L = top
    if n < seg:
        return None
    while L > seg and peak(L - seg, L) < thr:
        L -= seg
    if L < seg:
        return None
    return (0, n) if L == top else (0, L - seg)


def walk_head(m, seg, thr, peak):
    s = 0
    while s < m - seg and peak(s, s + seg) < thr:
        s += seg
    if s >= m - seg:
        return None
    return (0, m) if s == 0 else (s - seg, m)


def walk_both(n, seg, thr, peak, defect=None):
    t = walk_tail(n, seg, thr, peak, defect)
    if t is None:
        return None
    h = walk_head(t[1], seg, thr, peak)
    return None if h is None else (h[0], t[1])


def walk_long(n, seg, step, thr, peak):
    L = n
    while L > seg:
        if peak(L - seg, L) < thr:
            return True
        L -= step
    return False


def walk_frames(row, n, frame, shift, thr, defect=None):
    padded = np.pad(np.asarray(row)[:n], shift, mode="symmetric" if defect == "edge" else "reflect")
    if defect == "past_end":
        padded = np.concatenate([padded, np.asarray(row)[n:n + 3]])
    peak, out, start = row_peak(padded, padded.shape[0], "seam" if defect == "seam" else None), [], 0
    while start + frame <= n + 2 * shift:
        hi = start + frame
        if defect == "past_end" and hi == n + 2 * shift:
            hi += 3
        out.append(1 if peak(start, hi) > thr else 0)
        start += shift
    return out


def results(row, n, thr, defect=None, seg=SEG):
    """Every result of one clip (the first n samples of `row`) as a tuple of plain values: tail, head, both, flag, labels"""
    thr = np.asarray(row).dtype.type(thr)
    peak = row_peak(row, n, defect)
    step = int(LONG["sample_rate"])
    return (walk_tail(n, seg, thr, peak, defect), walk_head(n, seg, thr, peak), walk_both(n, seg, thr, peak, defect),
            walk_long(n, seg, step, thr, peak), walk_frames(row, n, FRAME, SHIFT, thr, defect) if n > SHIFT else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the clips of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def planted_positions(n):
    """Where one sample decides: the last index of a window and the first of the next, on the tail grid (which ends at n) and on the
    head grid (from 0), at the first and the last seam of each; indices 0, 1 and 441 (the left reflection); n - 1 and n - 2."""
    m, r = divmod(n, SEG)
    pos = {0, 1, SHIFT, n - 1, n - 2}
    for k in {1, m // 2, m - 1}:
        pos |= {r + k * SEG - 1, r + k * SEG, k * SEG - 1, k * SEG}
    return sorted(p for p in pos if 0 <= p < n)


def planted_clips(dtype):
    out = []
    for n in LENGTHS:
        for p in planted_positions(n):
            x = np.zeros(n, dtype=dtype)
            x[p] = 2 * THR
            out.append(x)
    return out


def speechlike(n, seed, dtype):
    """Bursts of "speech" between silences: stretches of exact zeros and of a hum below the threshold"""
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    pos = int(rng.integers(0, max(1, min(2500, n // 2))))
    while pos < n:
        burst = int(rng.integers(60, 2600))
        x[pos:pos + burst] = 0.3 * rng.standard_normal(burst)[:max(0, n - pos)]
        gap = int(rng.integers(200, 3000))
        if rng.random() < 0.5:
            x[pos + burst:pos + burst + gap] = rng.uniform(-0.8 * THR, 0.8 * THR, gap)[:max(0, n - pos - burst)]
        pos += burst + gap
    return x.astype(dtype)


def random_clips(dtype, count=320, seed=7):
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(900, 12000, size=count)]
    lens[:len(LENGTHS)] = LENGTHS
    return [speechlike(n, 1000 * seed + i, dtype) for i, n in enumerate(lens)]


def silent_clips(dtype):
    """All silent: exact zeros, and a hum below the threshold"""
    hum = np.random.default_rng(3).uniform(-0.8 * THR, 0.8 * THR, 5003).astype(dtype)
    return [np.zeros(3000, dtype=dtype), hum]


def none_case(x, thr=THR, seg=SEG):
    """Which of the None cases of trim_empty a clip lands in, or "" when it does not return None"""
    n = x.shape[0]
    t = x.dtype.type(thr)
    if walk_both(n, seg, t, row_peak(x, n)) is not None:
        return ""
    if n < seg:
        return "short"
    if n == seg:
        return "one_segment"
    if not np.max(np.abs(x)) >= t:
        return "silent"
    return "dropped"


def golden():
    return np.load(GOLDEN)
