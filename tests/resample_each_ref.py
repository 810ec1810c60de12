"""The recurrence csrc/resample.hip's k_resample_each keeps, restated in NumPy: output by output, the terms in ascending k, one
rounding per product and one per sum in the clip's dtype.  tests/test_resample_each_host.py shows it equal to
scipy.signal.resample_poly bit for bit, which pins the order the kernel must keep."""
from math import gcd

import numpy as np
from scipy.signal import firwin


def reduced(up, down):
    g = gcd(int(up), int(down))
    return int(up) // g, int(down) // g


def out_len(n_in, up, down):
    up, down = reduced(up, down)
    return -((-int(n_in) * up) // down)


def poly_ref(x, up, down):
    """resample_poly(x, up, down) of a 1-D float32 or float64 array: with t = n down + hl,
    y[n] = sum over ascending k, 0 <= k < len(x), 0 <= t - k up <= 2 hl, of acc = fl(acc + fl(x[k] h[t - k up])),
    h = fl(g T(up)), g = firwin(20 M + 1, 1 / M, ("kaiser", 5.0)).astype(T).  All outputs advance together, one term per step."""
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype in (np.float32, np.float64)
    up, down = reduced(up, down)
    if up == down:
        return x.copy()
    hl = 10 * max(up, down)
    h = firwin(2 * hl + 1, 1.0 / max(up, down), window=("kaiser", 5.0)).astype(x.dtype)
    h = h * x.dtype.type(up)
    n_in, n_out = x.shape[0], out_len(x.shape[0], up, down)
    t = np.arange(n_out, dtype=np.int64) * down + hl
    q = t // up
    k_lo = np.maximum(q - (2 * hl - (t - q * up)) // up, 0)
    cnt = np.maximum(np.minimum(q, n_in - 1) - k_lo + 1, 0)
    acc = np.zeros(n_out, dtype=x.dtype)
    for i in range(int(cnt.max()) if n_out else 0):
        live = i < cnt
        k = np.where(live, k_lo + i, 0)
        p = x[k] * h[np.where(live, t - k * up, 0)]
        acc = np.where(live, acc + p, acc)
    assert acc.dtype == x.dtype
    return acc
