"""CPU: the arithmetic of the device resampler (csrc/resample.hip) against scipy.signal.resample_poly, its host-side window rule,
and the kernel's assembly."""
import os
import re
import subprocess
import sys
from math import gcd

import numpy as np
import pytest
from scipy.signal import firwin, resample_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every pair the handlers meet: 8 .. 96 kHz -> 44.1 kHz, and 44.1 kHz -> 8 / 16 / 48 kHz
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 48000, 88200, 96000)
PAIRS = [(r, 44100) for r in RATES] + [(44100, 8000), (44100, 16000), (44100, 48000)]


def _pair(sr_in, sr_out):
    g = gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def _taps(up, down):
    m = max(up, down)
    h = firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    return h, 10 * m


def kernel_order(x, up, down):
    """The sum k_resample_poly forms, restated: per output n < ceil(n_in up / down), over ascending k with 0 <= k < n_in and
    0 <= n down + hl - k up <= 2 hl, acc = fl32(acc + fl32(x[k] * h[n down + hl - k up])) -- vectorised over n, one term at a time."""
    h, hl = _taps(up, down)
    n_in = x.shape[0]
    n_out = -(-n_in * up // down)
    t = np.arange(n_out, dtype=np.int64) * down + hl
    k_lo = np.maximum(-((2 * hl - t) // up), 0)
    k_hi = np.minimum(t // up, n_in - 1)
    acc = np.zeros(n_out, np.float32)
    for j in range(int((k_hi - k_lo).max()) + 1 if n_out else 0):
        k = k_lo + j
        live = k <= k_hi
        kk = np.where(live, k, 0)
        p = (x[kk] * h[np.where(live, t - kk * up, 0)]).astype(np.float32)
        acc = np.where(live, (acc + p).astype(np.float32), acc)
    return acc


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_kernel_order_equals_resample_poly(sr_in, sr_out):
    """The order the kernel keeps is resample_poly's, bit for bit: lengths 1, 2, below the half filter, and a few thousand."""
    up, down = _pair(sr_in, sr_out)
    hl = 10 * max(up, down)
    rng = np.random.default_rng(sr_in + sr_out)
    for n in sorted({1, 2, 3, max(1, hl // up - 1), hl // up, hl // up + 1, 257, 1000, 4001}):
        for x in (rng.uniform(-1, 1, n).astype(np.float32), np.where(rng.random(n) < 0.5, -1.0, 32767 / 32768).astype(np.float32)):
            want = resample_poly(x, up, down)
            got = kernel_order(x, up, down)
            assert want.dtype == np.float32 and np.array_equal(got, want), (sr_in, sr_out, n)


def test_out_len_and_window_rule():
    """vfx_resample_out_len = len(resample_poly), and vfx_resample_window's input range is exactly the union of what the outputs of
    the window read (sufficient and minimal) -- over random lengths, pairs and output windows."""
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import Engine
    lib = _lib.load()
    rng = np.random.default_rng(7)
    pairs = [_pair(a, b) for a, b in PAIRS] + [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(20)]
    for _ in range(300):
        up, down = pairs[int(rng.integers(len(pairs)))]
        g = gcd(up, down)
        n_in = int(rng.integers(0, 3000))
        n_out = int(lib.vfx_resample_out_len(n_in, up, down))
        if up == down:
            assert n_out == n_in
            continue
        if n_in:
            assert n_out == resample_poly(np.zeros(n_in, np.float32), up, down).shape[0], (n_in, up, down)
        o0 = int(rng.integers(0, n_out + 20))
        n = int(rng.integers(0, 700))
        k0, k1 = Engine.resample_window(n_in, down * 1000, up * 1000, o0, n)   # (rates: the pair up to a common factor)
        up, down = up // g, down // g
        hl = 10 * max(up, down)
        need = set()
        for o in range(o0, min(o0 + n, n_out)):
            t = o * down + hl
            need.update(range(max(0, -((2 * hl - t) // up)), min(n_in - 1, t // up) + 1))
        want = (min(need), max(need) + 1) if need else (0, 0)
        assert (k0, k1) == want and len(need) == k1 - k0, (n_in, up, down, o0, n)
    # a pair whose filter does not fit the kernel, and bad rates
    assert lib.vfx_resample_out_len(100, 44100, 44099) == -1
    assert lib.vfx_resample_out_len(100, 0, 3) == -1
    assert not Engine.resample_supported(44099, 44100)
    assert all(Engine.resample_supported(a, b) for a, b in PAIRS)


def test_window_is_sufficient_for_the_sum():
    """Outputs [o0, o0 + n) computed from the input with everything outside vfx_resample_window's range zeroed are the outputs of
    the whole signal."""
    from voicefixer_main_amd.engine import Engine
    rng = np.random.default_rng(11)
    for sr_in, sr_out in ((48000, 44100), (16000, 44100), (44100, 16000), (8000, 44100)):
        up, down = _pair(sr_in, sr_out)
        x = rng.uniform(-1, 1, 2500).astype(np.float32)
        full = kernel_order(x, up, down)
        for o0, n in ((0, 1), (0, 300), (777, 513), (full.shape[0] - 5, 40)):
            k0, k1 = Engine.resample_window(x.shape[0], sr_in, sr_out, o0, n)
            xw = np.zeros_like(x)
            xw[k0:k1] = x[k0:k1]
            assert np.array_equal(kernel_order(xw, up, down)[o0:o0 + n], full[o0:o0 + n]), (sr_in, sr_out, o0, n)


def test_resample_kernel_assembly(tmp_path):
    """k_resample_poly compiled for gfx950: no scratch, no FLAT memory instruction, the repository's store-hazard and in-flight
    checkers pass, and no fused multiply-add anywhere -- an FMA rounds once where scipy rounds twice, which breaks bit-identity."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "resample.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", out, os.path.join(ROOT, "voicefixer_main_amd", "csrc", "resample.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    kernels = re.findall(r"\n(_ZN3vfx15k_resample_poly\w+):.*?; ScratchSize: (\d+)", asm, re.S)
    assert kernels, "k_resample_poly not found"
    assert all(int(s) == 0 for _, s in kernels), kernels
    assert not re.search(r"\n\s*flat_", asm)
    assert not re.search(r"\bv_(fma|fmac|mac|pk_fma)_f32", asm)
    assert re.search(r"\bv_mul_f32", asm) and re.search(r"\bv_add_f32", asm)
    for checker in ("asm_inflight_check.py", "asm_store_hazard_check.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", checker), out], capture_output=True, text=True)
        assert r.returncode == 0, (checker, r.stdout[-2000:])
