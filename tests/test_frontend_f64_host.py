"""CPU: the float64 references of tests/test_gpu_frontend_launches.py (tests/frontend_f64.py) are the oracle's operations, the inputs
of the glue cases are built so that the defects they are there for would show, and the shapes of the cases reach the launch geometries
they are named after."""
import numpy as np
import torch

import frontend_f64 as R
from oracle import dsp, pipeline
from oracle import vocoder as voc


def _clip(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def test_stft_references_are_the_oracle_per_clip():
    clips = [_clip(n, i) for i, n in enumerate((1025, 1323, 2500))]
    T = R.frames(2500)
    ref = R.stft_ref_varlen(clips, T)
    for b, c in enumerate(clips):
        n = R.frames(c.shape[0])
        sp, mel = dsp.wav_to_mel(c[None, None].astype(np.float64))
        re, im = dsp.stft(c[None].astype(np.float64))
        assert np.array_equal(ref["sp"][b, :n], sp[0, 0]) and not ref["sp"][b, n:].any()
        assert np.allclose(ref["mel"][b, :n], mel[0, 0], rtol=1e-12, atol=0) and not ref["mel"][b, n:].any()
        # re = sp * cos, im = sp * sin: the STFT itself wherever the power is above the clamp
        assert np.abs(ref["re"][b, :n] - re[0]).max() < 1e-9 and np.abs(ref["im"][b, :n] - im[0]).max() < 1e-9
        # the explicit DFT of two frames (first and last: both reflected)
        dre, dim = dsp.stft_dft_matrix(c[None].astype(np.float64), [0, n - 1])
        assert np.abs(ref["re"][b, [0, n - 1]] - dre[0]).max() < 1e-9 and np.abs(ref["im"][b, [0, n - 1]] - dim[0]).max() < 1e-9
    chunked = R.stft_ref_chunked(np.stack([_clip(2500, 10 + i) for i in range(5)]), want=("mel", "sp"), chunk=2)
    whole = R.stft_ref(np.stack([_clip(2500, 10 + i) for i in range(5)]), want=("mel", "sp"))
    assert np.allclose(chunked["mel"], whole["mel"], rtol=1e-12, atol=0) and np.array_equal(chunked["sp"], whole["sp"])
    assert R.pad_rows([np.ones((2, 3)), np.ones((4, 3))], 3, -8.0).tolist() == [[[1] * 3, [1] * 3, [-8] * 3], [[1] * 3] * 3]


def test_istft_reference_inverts_the_rounded_spectrum():
    c = _clip(4533, 3)
    re, im = R.spectrum32(c)
    assert re.dtype == np.float32 and re.shape == (R.frames(4533), R.NBINS)
    back = R.istft_ref(re[None], im[None], 4533)[0]
    assert np.abs(back - c).max() < 1e-5        # the float32 rounding of the spectrum, nothing else
    assert np.array_equal(back, dsp.istft(re[None].astype(np.float64), im[None].astype(np.float64), 4533)[0])


def test_case_lengths():
    assert [R.frames(n) for n in R.EDGE_LENGTHS] == [3, 3, 4, 5, 5, 6, 11] and R.frames(R.L65) == 65 and R.L65 % R.HOP
    ln = R.f3_lengths()
    assert len(ln) == 80 and min(ln) == 1025 and max(ln) == R.L65
    assert {R.frames(n) % 3 for n in ln[:5]} == {0, 1, 2}
    ln = R.large_istft_lengths()
    assert len(ln) == 128 and min(ln) >= 1025 and R.frames(max(ln)) == 33
    assert 16 * R.HOP - 1025 in ln and 16 * R.HOP - 1023 in ln


def test_cases_reach_the_geometries_they_are_named_after():
    """Host-only queries of the launchers' own geometry functions (no GPU): frames per wave of the forward launches, IH of the inverse."""
    from voicefixer_main_amd.engine import Engine
    fpg = Engine.plan_stft_frames_per_group
    assert fpg(7 * 11) == 1 and fpg(1 * 65) == 1 and fpg(2048) == 1 and fpg(2049) == 2
    assert fpg(48 * 65) == 2 and -(-65 // 2) == 33 and 65 % 2 == 1          # 33 groups, the last one partial
    assert fpg(80 * 65) == 3
    assert fpg(225 * 65) == 8 == fpg(16 * 1001)                              # the benched 16 x 10 s launch
    assert fpg(1024 * 65) == 32 and -(-1024 * 65 // 2048) > 32               # capped
    assert Engine.plan_istft_grid(7, 11, 4533) == (2, -(-(1024 + 4533) // (2 * 441)))
    assert Engine.plan_istft_grid(128, 33, 14200) == (16, -(-(1024 + 14200) // (16 * 441)))
    assert Engine.plan_istft_grid(64, 64, 441 * 80) == (16, 6)
    assert Engine.plan_istft_grid(1, 64, 441 * 80)[0] == 2 and Engine.plan_istft_grid(1, 4095, 441 * 80)[0] == 2


def test_from_log_reference_and_inputs():
    x = R.from_log_inputs()
    assert x.shape == (3, 65, 128) and x.dtype == np.float32 and x.min() == -9.0 and x.max() == 6.5
    assert (x == 5.0).any() and (x > 5.0).sum() > 1000 and (x == np.nextafter(np.float32(5), np.float32(6))).any()
    ref = R.from_log(x)
    assert ref.dtype == np.float64 and ref.max() == 1e5 and (ref[x >= 5.0] == 1e5).all()
    assert np.allclose(ref, dsp.from_log(x), rtol=1e-5)       # the oracle in the input's precision
    assert np.array_equal(ref, 10.0 ** np.minimum(x.astype(np.float64), 5.0))


def test_unify_reference_is_amp_to_original_f_and_the_inputs_expose_an_off_by_one():
    for lens_t in (None, [65, 1, 37]):
        lg, tgt = R.unify_inputs(3, 65, lens_t)
        est = R.from_log(lg).astype(np.float32)
        ratio = R.unify_ratio(est, tgt, lens_t)
        for b in range(3):
            n = 65 if lens_t is None else lens_t[b]
            want, _ = pipeline.amp_to_original_f(est[b:b + 1, None, :n].astype(np.float64), tgt[b:b + 1, None, :n].astype(np.float64))
            assert np.allclose(want[0, 0], est[b, :n] * ratio[b], rtol=1e-12, atol=0)
            bound = R.unify_bound(n)
            assert bound == (40 * n + 2) * 2.0 ** -24
            # decoys: bins 4 and 25, and the frames past the clip, at least 100 times their neighbours -- in both tensors
            for t_ in (est, tgt):
                for edge in (4, 25):
                    assert (t_[b, :n, edge] >= 100 * np.maximum(t_[b, :n, edge - 1], t_[b, :n, edge + 1])).all()
                if n < 65:
                    assert (t_[b, n:] >= 100 * t_[b, :n].max(axis=0)).all()
            # spectral shape: the per-bin energy ratio target / estimate varies over the band (no single scale maps one to the other)
            shape = tgt[b, :n, 5:25].astype(np.float64).sum(0) / est[b, :n, 5:25].astype(np.float64).sum(0)
            assert shape.max() / shape.min() > 3
            # either band edge or the frame limit moved by one: far outside the bound of the GPU test
            moved = [R.unify_ratio(est, tgt, lens_t, lo=4)[b], R.unify_ratio(est, tgt, lens_t, lo=6)[b],
                     R.unify_ratio(est, tgt, lens_t, hi=24)[b], R.unify_ratio(est, tgt, lens_t, hi=26)[b]]
            if n > 1:
                moved.append(R.unify_ratio(est, tgt, lens_t, frame_shift=-1)[b])
            if n < 65:
                moved.append(R.unify_ratio(est, tgt, lens_t, frame_shift=1)[b])
            for m in moved:
                assert abs(m / ratio[b] - 1) > 10 * bound, (lens_t, b, m, ratio[b], bound)


def test_voc_prep_reference_and_inputs():
    cfg = voc.VocoderConfig()
    w = voc.mel_band_weight(128)
    for T in (65, 66):
        Tp = R.voc_tp(T)
        assert Tp == T + T % 2 + 4 == T + cfg.tail_frames(T)
        x = R.voc_prep_inputs(2, T)
        m = np.abs(x / w)
        assert (x == 0).any() and (x < 0).any() and ((m > 0) & (m < cfg.amp_floor)).any() and (m > 10.0).any()
        ref = R.voc_prep_ref(x, Tp)
        want = voc.normalise_mel(torch.from_numpy(x[:, None].astype(np.float64)), cfg).numpy().transpose(0, 2, 1)     # (B, Tp, 128)
        assert want.shape == ref.shape == (2, Tp, 128) and np.array_equal(ref, want)
        R_ = cfg.norm_range
        assert (ref[:, T:] == -R_).all() and (ref[:, 3] == R_).all() and (ref[:, 1] == -R_).all() and ref.min() == -R_ and ref.max() == R_
        assert ((ref > -R_) & (ref < R_)).mean() > 0.5        # most values are on the slope, not on a clamp
        # the float32 oracle agrees within its own rounding
        f32 = voc.normalise_mel(torch.from_numpy(x[:, None]), cfg).numpy().transpose(0, 2, 1)
        assert np.abs(f32 - ref).max() < 1e-4
        lens_t = [T, 9]
        refl = R.voc_prep_ref(x, Tp, lens_t)
        assert np.array_equal(refl[0], ref[0]) and np.array_equal(refl[1, :9], ref[1, :9]) and (refl[1, 9:] == -R_).all()


def test_peak_trim_reference_is_trim_center_of_peak_normalise():
    Llong = 70 * 441
    x = np.random.default_rng(5).uniform(-1.75, 1.75, size=(3, Llong)).astype(np.float32)
    peaks = [0.5, 1.0, 1.75]
    for L in (28241, 28240):
        out, divided = R.peak_trim_ref(x, L, peaks)
        assert divided.tolist() == [False, False, True]
        for b in range(3):
            xb = x[b].astype(np.float64)
            norm = xb / peaks[b] if peaks[b] > 1.0 else xb
            want, _ = pipeline.trim_center(norm[None], np.zeros((1, L)))
            assert np.array_equal(out[b], want[0])
    # with the clip's own peak: pipeline.peak_normalise
    pk = np.abs(x).max(axis=1)
    out, divided = R.peak_trim_ref(x, 28241, pk)
    assert divided.all()
    for b in range(3):
        want, _ = pipeline.trim_center(pipeline.peak_normalise(x[b].astype(np.float64))[None], np.zeros((1, 28241)))
        assert np.array_equal(out[b], want[0])
    # varlen: each clip is the fixed form of its own (lens_tp * hop) vocoder samples
    lens_l = [28241, 12345, 1025]
    lens_tp = [R.voc_tp(R.frames(n)) for n in lens_l]
    assert lens_tp == [70, 32, 8]
    out, divided = R.peak_trim_ref(x, 28241, [0.5, 2.0, 1.0], lens_l, lens_tp)
    assert divided.tolist() == [False, True, False]
    for b in range(3):
        one, _ = R.peak_trim_ref(x[b:b + 1, :lens_tp[b] * 441], lens_l[b], [[0.5, 2.0, 1.0][b]])
        assert np.array_equal(out[b, :lens_l[b]], one[0]) and not out[b, lens_l[b]:].any()
