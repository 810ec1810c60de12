"""CPU: the float64 restatement of the bandwidth detector (tests/band_f64.py) against the host form simulate.band_cutoff, the defects
the GPU tests (tests/test_gpu_band.py) must be able to see, the anchors of the exclusive-prefix reading, the C ABI's declaration, the
list layer of restore_prefiltered_list against a stub engine, and band.hip's register allocation."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import band_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def clips():
    return {n: ref.clip_for(n) for n in ref.LENGTHS}


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(0).standard_normal(30000).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host form and the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.LENGTHS)
def test_host_form_equals_the_restatement(clips, n):
    from voicefixer_main_amd import simulate
    x = clips[n]
    assert ref.frames(n) == 1 + n // 512
    want = ref.cutoff(x)
    assert 0 < want < 22050
    assert simulate.band_cutoff(x) == want                                   # float32 sums, the same decision: the margin covers them
    assert simulate.band_cutoff(torch.from_numpy(x), 44100, 0.95) == want
    assert simulate.band_cutoff(x, fs=16000) == ref.cutoff(x, 16000) == int(8000 * (ref.cut_bin(x) / 1025))
    assert simulate.band_cutoff_hz(ref.cut_bin(x), 44100) == want
    assert ref.decision_margin(x) > 0


def test_silence_and_white_noise(noise):
    from voicefixer_main_amd import simulate
    zeros = np.zeros(3000, np.float32)
    assert ref.cut_bin(zeros) == 0 and ref.cutoff(zeros) == 0 and simulate.band_cutoff(zeros) == 0
    assert not ref.profile(zeros).any()
    # white noise has the same energy in every bin: the EXCLUSIVE prefix over 1024 bins reaches 95 % at bin 974 (an inclusive one a bin
    # earlier), 20 952 Hz
    assert ref.cut_bin(noise) == 974 and ref.cutoff(noise) == 20952 == simulate.band_cutoff(noise)
    e = ref.profile(noise)
    assert ref.decide(e, inclusive=True)[0] == 973
    # threshold 1: the level is the total, which only P[1024] reaches
    assert ref.decide(e, 1.0)[0] == 1024


@pytest.mark.parametrize("n", ref.LENGTHS)
def test_planted_defects_move_the_profile_or_the_bin(clips, noise, n):
    x = clips[n]
    e, be = ref.profile(x), ref.energy_bound(x)
    i = ref.cut_bin(x)
    assert 0 < be < 1e-3 and e.max() > 1.0
    row = ref.L65 + 300                                                       # the padded batch of the GPU tests
    moved = lambda d: float(np.abs(d - e).max())
    assert moved(ref.profile(x, row=row)) > 100 * be                          # reflection at the row's end
    assert moved(ref.profile(x, row=row, row_frames=True)) > 100 * be         # ... and the batch's frame count
    assert moved(ref.profile(x, eps=1e-8)) > 10 * be                          # the clamp left in: 1e-4 in every empty bin
    assert moved(ref.profile(x, hop=441)) > 100 * be                          # the handlers' hop in place of librosa's
    assert ref.decide(e, inclusive=True)[0] == i - 1                          # an inclusive prefix: a bin earlier
    # bin 1024 counted: these clips have nothing up there, white noise has
    assert ref.decide(ref.profile(noise), count_top=True)[0] == 975


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI as declared
# ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_and_bound():
    from voicefixer_main_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vfx.h")).read()
    m = re.search(r"\bint vfx_band_energy\(([^;]*)\);", hdr)
    assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == 10 == len(_lib.SIGNATURES["vfx_band_energy"][1])
    assert _lib.SIGNATURES["vfx_band_energy"][1][6] is __import__("ctypes").c_double          # threshold
    assert re.search(r"#define VFX_BAND_BINS 1025\b", hdr) and _lib.BAND_BINS == 1025
    mk = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bband\.hip\b", mk, re.M)
    # the shared front end is ONE text: band.hip includes it and restates nothing of the transform
    src = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "band.hip")).read()
    assert '#include "stft_wave.h"' in src and "void wfft1024(" not in src and "#pragma clang fp contract(off)" in src
    assert "atomicAdd" not in src and "unsafeAtomicAdd" not in src
    assert src.count("__syncthreads") == 4          # one after k_band_energy's table load, three in k_band_cut


# ---------------------------------------------------------------------------------------------------------------------------------
# restore_prefiltered_list against a stub engine
# ---------------------------------------------------------------------------------------------------------------------------------
class _Cfg:
    sample_rate = 44100


class _StubEngine:
    device = torch.device("cpu")
    cfg = _Cfg()


def test_restore_prefiltered_list_order_and_silent_clip(monkeypatch):
    from voicefixer_main_amd import models, simulate
    calls = {"detect": [], "lowpass": [], "restore": []}
    # a clip's "cut-off" = 100 x its first sample; a clip that starts with 0 is "silent"
    def band_cutoff_list(clips, fs=44100, threshold=0.95, engine=None):
        calls["detect"].append((len(clips), fs, threshold, engine))
        return [int(100 * float(c[0])) for c in clips]

    def lowpass_each(clips, highcuts, fs, orders=5, types="butter", engine=None, to_host=True):
        calls["lowpass"].append(([float(c[0]) for c in clips], list(highcuts), fs, orders, types, engine, to_host))
        return [c + 0.5 for c in clips]

    monkeypatch.setattr(simulate, "band_cutoff_list", band_cutoff_list)
    monkeypatch.setattr(simulate, "lowpass_each", lowpass_each)
    for cls, kwargs in ((models.VoiceFixer, dict(unify_energy=True, max_batch=3)), (models.SSR_UNet, dict(max_batch=2))):
        for v in calls.values():
            del v[:]
        eng = _StubEngine()
        m = object.__new__(cls)
        m.engine, m.device = eng, eng.device

        def restore_list(wavs, **kw):
            calls["restore"].append(([float(w[0]) for w in wavs], kw))
            return [w * 2 for w in wavs]
        m.restore_list = restore_list
        wavs = [torch.full((5,), 3.0), np.zeros(4, np.float32), torch.full((6,), 1.0), torch.full((3,), 2.0)]
        out, cutoffs = m.restore_prefiltered_list(wavs, threshold=0.9, **kwargs)
        assert cutoffs == [300, 0, 100, 200]                                                    # input order
        assert calls["detect"] == [(4, 44100, 0.9, eng)]
        # one cut-off per clip with content, type "stft", order 5, results kept on the device; the silent clip is not filtered
        assert calls["lowpass"] == [([3.0, 1.0, 2.0], [300, 100, 200], 44100, 5, "stft", eng, False)]
        assert calls["restore"] == [([3.5, 0.0, 1.5, 2.5], kwargs)]                             # once, with the filtered clips
        assert [float(o[0]) for o in out] == [7.0, 0.0, 3.0, 5.0] and [o.shape[0] for o in out] == [5, 4, 6, 3]
        # nothing to filter: lowpass_each is not called
        out, cutoffs = m.restore_prefiltered_list([torch.zeros(4)])
        assert cutoffs == [0] and len(calls["lowpass"]) == 1 and calls["detect"][-1][2] == 0.95


def test_band_cutoff_list_batches_by_length():
    from voicefixer_main_amd import simulate

    class Eng:
        device = torch.device("cpu")
        calls = []

        def band_cutoff(self, x, lengths=None, sample_rate=44100, hop=512, threshold=0.95):
            assert x.dtype == torch.float32 and x.shape == (len(lengths), max(lengths)) and hop == 512
            for j, n in enumerate(lengths):
                assert not x[j, n:].any()
            self.calls.append((list(lengths), sample_rate, threshold))
            return [int(x[j, 0]) for j in range(len(lengths))]
    eng = Eng()
    lens = [3000, 1025, 5000, 1030]
    clips = [np.full(n, float(k + 1)) for k, n in enumerate(lens)] + [np.zeros(1024, np.float32)]
    got = simulate.band_cutoff_list(clips, 16000, 0.5, engine=eng)
    assert got == [1, 2, 3, 4, 0]                                           # the caller's order; the short clip on the host
    assert eng.calls == [([1025, 1030, 3000, 5000], 16000, 0.5)]
    with pytest.raises(ValueError, match="1d time array"):
        simulate.band_cutoff_list([np.zeros((2000, 1))], engine=eng)
    assert simulate.band_cutoff_list([], engine=eng) == []


# ---------------------------------------------------------------------------------------------------------------------------------
# band.hip on gfx950: no spills
# ---------------------------------------------------------------------------------------------------------------------------------
def test_band_kernels_do_not_spill(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "band.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", out, os.path.join(ROOT, "voicefixer_main_amd", "csrc", "band.hip")],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    kernels = dict(re.findall(r"\n(_ZN3vfx\w+):.*?; ScratchSize: (\d+)", asm, re.S))
    for name in ("k_band_energy", "k_band_cut"):
        assert any(name in k for k in kernels), (name, list(kernels))
    for k, scratch in kernels.items():
        assert int(scratch) == 0, (k, scratch)
