"""CPU: what the list functions hand an Engine and how they hand the rows back -- the padded batches of simulate.reverb_rir_list,
add_noise_and_scale*_list and lowpass_list(_type="stft"), and of models._resample_list.  A stand-in engine on the CPU records its calls
and computes with SciPy / NumPy (the idea of tests/test_sosfiltfilt_host.py::HostEngine, which pins the IIR path)."""
import os
import sys
import types

import numpy as np
import pytest
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, models, simulate  # noqa: E402
from voicefixer_main_amd.engine import Engine  # noqa: E402

FS = 44100
LENGTHS = (902, 300, 2001, 301, 300)
F64 = 3      # the one clip that is not float32: it takes the host function
RIR_TAPS = (7, 33, 5)
RIR_INDEX = [2, 0, 2, 1, 2]
MIX_KW = dict(snr_l=-5, snr_h=30, scale_lower=0.5, scale_upper=0.9)
MIX_FORMS = [      # (list form, single-clip form, the engine's names of the signals)
    (simulate.add_noise_and_scale_list, simulate.add_noise_and_scale, ("front", "noise")),
    (simulate.add_noise_and_scale_with_HQ_list, simulate.add_noise_and_scale_with_HQ, ("hq", "front", "noise")),
    (simulate.add_noise_and_scale_with_HQ_with_Aug_list, simulate.add_noise_and_scale_with_HQ_with_Aug, ("hq", "front", "aug", "noise")),
]


def _clips(seed, lengths=LENGTHS, f64=(F64,)):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 0.3).astype(np.float64 if i in f64 else np.float32) for i, n in enumerate(lengths)]


def _mix_row(name, sig, weight, scale):
    """the stand-in's arithmetic for one clip: float32, one operation per step"""
    y = sig[name] / np.float32(weight) if name == "noise" and weight is not None else sig[name]
    return y * np.float32(scale)


class HostEngine:
    """What the list functions need of an Engine, computed on the host; records what it was handed."""
    device = torch.device("cpu")
    MAX_RIR_TAPS = Engine.MAX_RIR_TAPS
    cfg = types.SimpleNamespace(sample_rate=FS)

    def __init__(self):
        self.calls = []

    def reverb_rir(self, x, rirs, rir_index=None, lengths=None, rir_lengths=None, normalize=True):
        self.calls.append(dict(x=tuple(x.shape), dtype=x.dtype, lengths=list(lengths), bank=tuple(rirs.shape), rir_index=list(rir_index),
                               rir_lengths=list(rir_lengths)))
        y = torch.zeros(x.shape, dtype=torch.float32)
        for b, n in enumerate(lengths):
            r = rir_index[b]
            y[b, :n] = torch.from_numpy(simulate.reverb_rir(x[b, :n].numpy(), rirs[r, :rir_lengths[r]].numpy()).copy())
        return y, torch.zeros(len(lengths))

    def mix_noise(self, front, noise, hq=None, aug=None, lengths=None, noise_weight=None, scale=None, want_noisy=False):
        sig = {k: v for k, v in (("front", front), ("noise", noise), ("hq", hq), ("aug", aug)) if v is not None}
        self.calls.append(dict(shapes={k: tuple(v.shape) for k, v in sig.items()}, lengths=list(lengths),
                               noise_weight=None if noise_weight is None else list(noise_weight), scale=list(scale)))
        out = {k: torch.zeros(front.shape, dtype=torch.float32) for k in list(sig) + (["noisy"] if want_noisy else [])}
        for b, n in enumerate(lengths):
            row = {k: v[b, :n].numpy() for k, v in sig.items()}
            w = None if noise_weight is None else noise_weight[b]
            for k in sig:
                out[k][b, :n] = torch.from_numpy(_mix_row(k, row, w, scale[b]))
            if want_noisy:
                out["noisy"][b, :n] = out["noise"][b, :n] + out["aug" if aug is not None else "front"][b, :n]
        return out

    def resample(self, x, sr_in, sr_out, lengths=None):
        up, down = Engine.resample_ratio(sr_in, sr_out)
        self.calls.append(dict(x=tuple(x.shape), dtype=x.dtype, rates=(sr_in, sr_out), lengths=list(lengths)))
        rows = [signal.resample_poly(x[b, :n].numpy(), up, down) for b, n in enumerate(lengths)]
        y = torch.zeros((len(rows), max(len(r) for r in rows)), dtype=torch.float32)
        for b, r in enumerate(rows):
            y[b, :len(r)] = torch.from_numpy(r.copy())
        return y, [len(r) for r in rows]


@pytest.fixture
def small_batches(monkeypatch):
    monkeypatch.setattr(simulate, "MAX_BATCH", 2)


def _host(y):
    return y.numpy() if isinstance(y, torch.Tensor) else y


# ---------------------------------------------------------------------------------------------------------------- reverb_rir_list
def test_reverb_rir_list_batches(small_batches):
    clips = _clips(1)
    rirs = [np.random.default_rng(10 + k).standard_normal(m).astype(np.float32) * 0.2 for k, m in enumerate(RIR_TAPS)]
    eng = HostEngine()
    got = simulate.reverb_rir_list(clips, rirs, rir_index=RIR_INDEX, engine=eng)
    assert eng.calls == [
        dict(x=(2, 300), dtype=torch.float32, lengths=[300, 300], bank=(2, 7), rir_index=[0, 1], rir_lengths=[7, 5]),
        dict(x=(2, 2001), dtype=torch.float32, lengths=[902, 2001], bank=(1, 5), rir_index=[0, 0], rir_lengths=[5]),
    ]
    want = [simulate.reverb_rir(c, rirs[r]) for c, r in zip(clips, RIR_INDEX)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == (np.float64 if i == F64 else np.float32)
        assert g.shape == (LENGTHS[i],) and np.array_equal(g, w)
    got[0][:] = 0.0      # a host row is its own copy, not a view of the batch
    assert np.array_equal(got[2], want[2])
    dev = simulate.reverb_rir_list(clips, rirs, rir_index=RIR_INDEX, engine=eng, to_host=False)
    assert len(eng.calls) == 4
    for g, w in zip(dev, want):
        assert isinstance(g, torch.Tensor) and g.device == eng.device and np.array_equal(g.numpy(), w)
    # one RIR for every clip, default index
    eng = HostEngine()
    got = simulate.reverb_rir_list(clips[:2], rirs[1], engine=eng)
    assert eng.calls == [dict(x=(2, 902), dtype=torch.float32, lengths=[300, 902], bank=(1, 33), rir_index=[0, 0], rir_lengths=[33])]
    assert all(np.array_equal(g, simulate.reverb_rir(c, rirs[1])) for g, c in zip(got, clips))


# ---------------------------------------------------------------------------------------------------------------- add_noise_and_scale*_list
@pytest.mark.parametrize("list_fn, one_fn, names", MIX_FORMS)
@pytest.mark.parametrize("to_host", [True, False])
def test_mix_list_batches_and_draws(small_batches, list_fn, one_fn, names, to_host):
    nsig = len(names)
    sig = [_clips(20 + k) for k in range(nsig)]
    eng = HostEngine()
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    got = list_fn(*sig, rng=a, engine=eng, to_host=to_host, want_noisy=True, **MIX_KW)
    # the draws of a loop over the single-clip rule: snr then scale per item, the host item's inside its own function
    draws, host_item = [], None
    for i in range(len(LENGTHS)):
        if i == F64:
            host_item = one_fn(*[s[i] for s in sig], rng=b, **MIX_KW)
            draws.append(tuple(host_item[nsig:]))
        else:
            snr = simulate._uniform(MIX_KW["snr_l"], MIX_KW["snr_h"], b)
            draws.append((snr, simulate._uniform(MIX_KW["scale_lower"], MIX_KW["scale_upper"], b)))
    assert a.random() == b.random()
    assert len(set(draws)) == len(draws)
    batches = [[1, 4], [0, 2]]
    assert eng.calls == [
        dict(shapes={k: (2, w) for k in names}, lengths=[LENGTHS[i] for i in idx],
             noise_weight=[10 ** (float(draws[i][0]) / 20) for i in idx], scale=[draws[i][1] for i in idx])
        for idx, w in zip(batches, (300, 2004))]
    speech = "aug" if "aug" in names else "front"
    for i, t in enumerate(got):
        assert len(t) == nsig + 3 and t[nsig:nsig + 2] == draws[i]
        ys = [t[k] for k in list(range(nsig)) + [nsig + 2]]
        if to_host:
            assert all(isinstance(y, np.ndarray) for y in ys)
        else:
            assert all(isinstance(y, torch.Tensor) and y.device == eng.device for y in ys)
        ys = [_host(y) for y in ys]
        assert all(y.shape == (LENGTHS[i],) for y in ys)
        if i == F64:
            want = list(host_item[:nsig])
            want.append(want[names.index("noise")] + want[names.index(speech)])
            assert all(y.dtype == np.float64 for y in ys)
        else:
            row = {k: s[i] for k, s in zip(names, sig)}
            want = [_mix_row(k, row, 10 ** (float(draws[i][0]) / 20), draws[i][1]) for k in names]
            want.append(want[names.index("noise")] + want[names.index(speech)])
            assert all(y.dtype == np.float32 for y in ys)
        assert all(np.array_equal(y, w) for y, w in zip(ys, want))


def test_mix_list_without_snr_passes_no_weight(small_batches):
    sig = [_clips(30), _clips(31)]
    eng = HostEngine()
    got = simulate.add_noise_and_scale_list(*sig, snr_l=None, snr_h=30, scale_lower=0.7, scale_upper=0.7, engine=eng)
    assert [c["noise_weight"] for c in eng.calls] == [None, None] and [c["scale"] for c in eng.calls] == [[0.7, 0.7]] * 2
    assert all(len(t) == 4 and t[2] is None and t[3] == 0.7 for t in got)


def test_mix_list_host_only_creates_no_engine(monkeypatch):
    def boom():
        raise AssertionError("the host path must not create an Engine")
    monkeypatch.setattr(simulate, "_get_engine", boom)
    for list_fn, one_fn, names in MIX_FORMS:
        sig = [_clips(40 + k, lengths=(300, 0, 64), f64=(0, 1, 2)) for k in range(len(names))]
        for s in sig:
            s[1] = s[1].astype(np.float32)      # an EMPTY float32 item takes the host function as well (and fails as it does)
        with pytest.raises(ValueError):
            list_fn(*sig, rng=np.random.default_rng(0), to_host=True)
        sig = [[s[0], s[2]] for s in sig]
        got = list_fn(*sig, rng=np.random.default_rng(0), to_host=True, want_noisy=True)
        b = np.random.default_rng(0)
        for i, t in enumerate(got):
            want = one_fn(*[s[i] for s in sig], rng=b)
            assert all(np.array_equal(g, w) for g, w in zip(t[:len(names)], want)) and t[len(names):-1] == want[len(names):]


# ---------------------------------------------------------------------------------------------------------------- lowpass_list, "stft"
def test_stft_list_resamples_down_and_up(small_batches):
    try:
        _lib.load()      # Engine.resample_supported asks the library which rate pairs its kernel takes
    except RuntimeError as e:
        pytest.skip(str(e))
    highcut, fs_down = 11025, 22050
    assert int(highcut / int(FS / 2) * FS) == fs_down and Engine.resample_supported(FS, fs_down) and Engine.resample_supported(fs_down, FS)
    clips = _clips(2)
    eng = HostEngine()
    got = simulate.lowpass_list(clips, highcut, FS, _type="stft", engine=eng)
    low = lambda n: -(-n // 2)
    assert eng.calls == [
        dict(x=(2, 300), dtype=torch.float32, rates=(FS, fs_down), lengths=[300, 300]),
        dict(x=(2, 150), dtype=torch.float32, rates=(fs_down, FS), lengths=[150, 150]),
        dict(x=(2, 2001), dtype=torch.float32, rates=(FS, fs_down), lengths=[902, 2001]),
        dict(x=(2, low(2001)), dtype=torch.float32, rates=(fs_down, FS), lengths=[low(902), low(2001)]),
    ]
    want = [simulate.lowpass(c, highcut, FS, _type="stft") for c in clips]
    for i, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == (np.float64 if i == F64 else np.float32)
        assert g.shape == (LENGTHS[i],) and np.array_equal(g, w)
    dev = simulate.lowpass_list(clips, highcut, FS, _type="stft", engine=eng, to_host=False)
    for g, w in zip(dev, want):
        assert isinstance(g, torch.Tensor) and g.device == eng.device and np.array_equal(g.numpy(), w)
    # a rate pair the device does not take, and an empty clip: the host function, no engine call
    eng = HostEngine()
    odd = simulate.lowpass_list(clips[:2], 4001, FS, _type="stft", engine=eng)
    if not Engine.resample_supported(FS, int(4001 / int(FS / 2) * FS)):
        assert eng.calls == []
    assert all(np.array_equal(g, simulate.lowpass(c, 4001, FS, _type="stft")) for g, c in zip(odd, clips))


def test_stft_hard_list_converts_once_per_clip():
    """`stft_hard` of a list: every clip through the single-clip function on the one engine, tensors or arrays in, the caller's order."""
    class Stft:
        device = torch.device("cpu")

        def stft(self, x, want_mel, want_sp, want_phase):
            sp = x[:, :, None].abs().repeat(1, 1, 4)
            return dict(sp=sp, cos=torch.ones_like(sp), sin=torch.zeros_like(sp))

        def istft(self, re, im, length):
            return re.sum(-1)[:, :length]

    clips = _clips(3, lengths=(50, 20, 50))
    eng = Stft()
    want = [simulate.lowpass(c, 11025, FS, _type="stft_hard", engine=eng) for c in clips]
    assert not np.array_equal(want[0], want[2])
    got = simulate.lowpass_list([clips[0], torch.from_numpy(clips[1]), clips[2]], 11025, FS, _type="stft_hard", engine=eng)
    assert all(isinstance(g, np.ndarray) and np.array_equal(g, w) for g, w in zip(got, want))
    dev = simulate.lowpass_list(clips, 11025, FS, _type="stft_h",engine=eng, to_host=False)
    assert all(isinstance(g, torch.Tensor) and np.array_equal(g.numpy(), w) for g, w in zip(dev, want))


# ---------------------------------------------------------------------------------------------------------------- models._resample_list
def test_resample_list_is_one_padded_batch():
    eng = HostEngine()
    wavs = [torch.from_numpy(c) for c in _clips(4)]
    got = models._resample_list(eng, wavs, 16000)
    assert eng.calls == [dict(x=(5, 2001), dtype=torch.float32, rates=(16000, FS), lengths=list(LENGTHS))]
    for g, w in zip(got, wavs):
        want = signal.resample_poly(w.numpy().astype(np.float32), 441, 160)
        assert g.dtype == torch.float32 and g.shape == want.shape and np.array_equal(g.numpy(), want)
    # (1, L) clips are flattened
    eng = HostEngine()
    again = models._resample_list(eng, [w[None] for w in wavs], 16000)
    assert eng.calls[0]["x"] == (5, 2001) and all(np.array_equal(g.numpy(), h.numpy()) for g, h in zip(again, got))
    # nothing to do: the very list comes back, and the engine is not asked
    eng = HostEngine()
    empty = []
    assert models._resample_list(eng, empty, 16000) is empty and models._resample_list(eng, wavs, FS) is wavs and eng.calls == []


# ---------------------------------------------------------------------------------------------------------------- order stability
def test_equal_lengths_keep_the_callers_positions(small_batches):
    """Two clips of one length and different contents, a shorter and a longer one around them: ties keep the caller's order inside a
    batch, and every row goes back to its own position."""
    lengths = (400, 350, 400, 300)
    clips = _clips(6, lengths=lengths, f64=())
    assert not np.array_equal(clips[0], clips[2])
    rir = np.random.default_rng(7).standard_normal(9).astype(np.float32) * 0.2
    for to_host in (True, False):
        eng = HostEngine()
        got = simulate.reverb_rir_list(clips, [rir], engine=eng, to_host=to_host)
        assert [c["lengths"] for c in eng.calls] == [[300, 350], [400, 400]]
        assert all(np.array_equal(_host(g), simulate.reverb_rir(c, rir)) for g, c in zip(got, clips))

        eng = HostEngine()
        noise = _clips(8, lengths=lengths, f64=())
        got = simulate.add_noise_and_scale_list(clips, noise, snr_l=None, snr_h=None, scale_lower=1.0, scale_upper=1.0, engine=eng,
                                                to_host=to_host)
        assert [c["lengths"] for c in eng.calls] == [[300, 350], [400, 400]]
        assert all(np.array_equal(_host(t[0]), c) and np.array_equal(_host(t[1]), n) for t, c, n in zip(got, clips, noise))

        from test_sosfiltfilt_host import HostEngine as SosEngine
        eng = SosEngine()
        got = simulate.lowpass_list(clips, 1000, FS, engine=eng, to_host=to_host)
        assert [c[2] for c in eng.calls] == [[300, 350], [400, 400]]
        assert all(np.array_equal(_host(g), simulate.lowpass(c, 1000, FS)) for g, c in zip(got, clips))
        got = simulate.bandpass_list(clips, 300, 3400, FS, engine=eng, to_host=to_host)
        assert all(np.array_equal(_host(g), simulate.bandpass(c, 300, 3400, FS)) for g, c in zip(got, clips))

        got = simulate.hard_clip_list(clips, 0.1, engine=HostEngine(), to_host=to_host)
        assert all(np.array_equal(_host(g), simulate.hard_clip(c, 0.1)) for g, c in zip(got, clips))

    eng = HostEngine()
    got = models._resample_list(eng, [torch.from_numpy(c) for c in clips], 22050)
    assert eng.calls[0]["lengths"] == list(lengths)
    assert all(np.array_equal(g.numpy(), signal.resample_poly(c, 2, 1)) for g, c in zip(got, clips))


def test_equal_lengths_keep_the_callers_positions_stft(small_batches):
    try:
        _lib.load()
    except RuntimeError as e:
        pytest.skip(str(e))
    clips = _clips(6, lengths=(400, 350, 400, 300), f64=())
    eng = HostEngine()
    got = simulate.lowpass_list(clips, 11025, FS, _type="stft", engine=eng)
    assert [c["lengths"] for c in eng.calls[::2]] == [[300, 350], [400, 400]]
    assert all(np.array_equal(g, simulate.lowpass(c, 11025, FS, _type="stft")) for g, c in zip(got, clips))


# ---------------------------------------------------------------------------------------------------------------- the helpers themselves
def test_clips_module():
    from voicefixer_main_amd import clips
    lengths = [5, 3, 5, 1, 3]
    assert list(clips.batches(range(5), lengths, 2)) == [[3, 1], [4, 0], [2]]
    assert list(clips.batches([4, 1], lengths, 8)) == [[4, 1]] and list(clips.batches([], lengths, 8)) == []
    rows = [np.arange(3, dtype=np.float64), torch.arange(5, dtype=torch.float32)[::2], np.zeros(0, np.float32)]
    x = clips.pad(rows, torch.device("cpu"), torch.float32)
    assert x.dtype == torch.float32 and x.tolist() == [[0, 1, 2], [0, 2, 4], [0, 0, 0]]
    assert clips.pad(rows, torch.device("cpu"), torch.float64, width=4).shape == (3, 4)
    host, dev = clips.unpad(x, [3, 2, 0], True), clips.unpad(x, [3, 2, 0], False)
    assert [h.tolist() for h in host] == [d.tolist() for d in dev] == [[0, 1, 2], [0, 2], []]
    x[0, 0] = 9.0      # host rows are copies, device rows views
    assert host[0][0] == 0.0 and dev[0][0] == 9.0
    a = np.ones((4, 2), np.float32)[:, 0]
    assert clips.as_tensor(a).tolist() == [1.0] * 4 and clips.as_numpy(a) is a and clips.as_tensor(x) is x
    assert clips.is_f32(a) and clips.is_f32(x) and not clips.is_f32(rows[0]) and not clips.is_f32(torch.zeros(1, dtype=torch.float64))
    assert clips.to_device(a, "cpu").dtype == torch.float32 and np.array_equal(clips.as_numpy(clips.to_device(a, "cpu")), a)


def test_engine_clip_rows():
    """The argument handling the Engine's clip-batch methods share: 1-D x is one clip, lengths default to the row length, and the
    count is checked under the method's name."""
    from voicefixer_main_amd.engine import _clip_rows
    x = torch.zeros(3, 7)
    x2, squeeze, B, L, lengths = _clip_rows(x, None, "resample")
    assert x2 is x and not squeeze and (B, L, lengths) == (3, 7, [7, 7, 7])
    x2, squeeze, B, L, lengths = _clip_rows(x[0], np.array([5.0]), "resample")
    assert x2.shape == (1, 7) and squeeze and (B, L, lengths) == (1, 7, [5]) and type(lengths[0]) is int
    with pytest.raises(ValueError, match=r"^sosfiltfilt: 2 lengths for 3 clips$"):
        _clip_rows(x, [1, 2], "sosfiltfilt")
    with pytest.raises(ValueError, match=r"^analysis_mel: 4 frame counts for 3 clips$"):
        _clip_rows(x, [1, 2, 3, 4], "analysis_mel", "frame counts")
    assert _clip_rows(x, [1, 2])[4] == [1, 2]      # no name: the caller words its own check
    with pytest.raises(ValueError):
        _clip_rows(torch.zeros(2, 3, 4), None, "resample")
