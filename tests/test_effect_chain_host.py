"""Host side of the effect chain (simulate.biquad_design, chain_effects, magical_effects, draw_effects): the designs against
scipy.signal.butter and against their own definition (the shelves' gain at DC and Nyquist, the poles), `chain_effects` bit for bit
against the recurrence, the clamp and the flip written out here, the saturation at sox's sample range, `magical_effects` as the
composition of the chain and the `array_effects` tail, the draws against a loop that mirrors RandomServer.do, and the binding of
vfx_effect_chain.  The chain is RESTATED from published definitions, not pinned against sox: nothing here compares with sox.
No GPU, no Engine."""
import cmath
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicefixer_main_amd import _lib, simulate  # noqa: E402

FS = 44100
LO, HI = -1.0, 1.0 - 2.0 ** -31
NOT_BUILT = ("tempo", "speed", "pitch", "fade", "tremolo", "reverb_freeverb")
# RandomServer's defaults with the values of config/vctk_base_voicefixer_unet.json where it sets the name (its low_pass ranges are
# those of "low_pass_1" / "low_pass_2", which RandomServer.do does not know: "low_pass" keeps the default); the two-entry `prob` lists
# are 0.8 / 0.4 so that one chance picks the up range and another the down range
P_EFFECTS = {
    "tempo": {"prob": [0.8, 0.4], "speed_up_range": [1.1, 1.6], "speed_down_range": [0.7, 0.95]},
    "speed": {"prob": [0.8, 0.4], "speed_up_range": [1.1, 1.6], "speed_down_range": [0.7, 0.95]},
    "fade": {"prob": [0.1], "fade_in_portion": [0.1, 0.3], "fade_out_portion": [0.1, 0.3]},
    "pitch": {"prob": [0.8, 0.4], "pitch_up_range": [100, 350], "pitch_down_range": [-350, -100]},
    "treble": {"prob": [0.05], "level": [3, 20]},
    "bass": {"prob": [0.15], "level": [3, 35]},
    "tremolo": {"prob": [0.3], "level": [5, 50]},
    "reverb_freeverb": {"prob": [0.20], "reverb_level": [0, 50], "dumping_factor": [0, 100], "room_size": [0, 100]},
    "reverb_rir": {"prob": [0.30], "rir_file_name": ""},
    "low_pass": {"prob": [0.3], "low_pass_range": [3000, 7000]},
    "high_pass": {"prob": [0.25], "high_pass_range": [500, 2000]},
    "clip": {"prob": [0.20], "louder_time": [1.0, 11.0]},
    "reverse": {"prob": [0.1]},
    "time_dropout": {"prob": [0.1], "max_segment": 0.1, "drop_range": [0.0, 1.0]},
    "quant": {"prob": [0.2], "bins": [3, 12]},
    "empty_c": {"prob": [0.2]},
    "empty_n": {"prob": [1.0]},
    "anytime": {"prob": [0.5], "inner_segment_scale": [0.1, 1.0], "overall_scale": [0.6, 1.0], "first_segment_portion": [0.25, 0.75],
                "snr_range": [-5, 45]},
}


def seeded(n, seed, scale=0.5):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# designs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [500, 3000, 7000, 21000])
@pytest.mark.parametrize("name, btype", [("low_pass", "low"), ("high_pass", "high")])
def test_butterworth_designs_equal_scipy(name, btype, f):
    from scipy.signal import butter
    b, a = butter(2, f, btype, fs=FS)
    got = np.array(simulate.biquad_design(name, f))
    assert np.abs(got - np.r_[b, a[1:]]).max() <= 1e-12


def _gain_db(design, z):
    b0, b1, b2, a1, a2 = design
    return 20 * math.log10(abs((b0 + b1 / z + b2 / z ** 2) / (1 + a1 / z + a2 / z ** 2)))


@pytest.mark.parametrize("gain", [3, 20, 35, -12])
def test_shelves_have_their_gain_at_one_end_and_none_at_the_other(gain):
    bass, treble = simulate.biquad_design("bass", gain), simulate.biquad_design("treble", gain)
    assert abs(_gain_db(bass, 1.0) - gain) <= 1e-9 and abs(_gain_db(bass, -1.0)) <= 1e-9
    assert abs(_gain_db(treble, -1.0) - gain) <= 1e-9 and abs(_gain_db(treble, 1.0)) <= 1e-9


def test_designs_are_stable_and_checked():
    designs = [simulate.biquad_design(n, f) for n in ("low_pass", "high_pass") for f in (20, 500, 3000, 7000, 21000, 22049)]
    designs += [simulate.biquad_design(n, g) for n in ("bass", "treble") for g in (-35, -3, 3, 20, 35)]
    for _, _, _, a1, a2 in designs:
        disc = cmath.sqrt(a1 * a1 - 4 * a2)
        assert max(abs((-a1 + disc) / 2), abs((-a1 - disc) / 2)) < 1
    assert simulate.biquad_design("bass", 0) == (1.0, 0.0, 0.0, 0.0, 0.0) == simulate.biquad_design("treble", 0.0)
    for name, value in (("low_pass", FS / 2), ("high_pass", 30000), ("low_pass", 0), ("high_pass", -5)):
        with pytest.raises(ValueError):
            simulate.biquad_design(name, value)
    with pytest.raises(ValueError):
        simulate.biquad_design("bass", 6, fs=150)      # the shelf's 100 Hz against fs / 2 = 75
    with pytest.raises(ValueError):
        simulate.biquad_design("clip", 2)


# ----------------------------------------------------------------------------------------------------------------------
# chain_effects: the recurrence, the clamp and the flip, written out
# ----------------------------------------------------------------------------------------------------------------------
def limit(v):
    return LO if v < LO else (HI if v > HI else v)


def biquad_loop(w, design):
    """One biquad over a list of Python floats (float64, every product and sum rounded on its own) -> the limited outputs"""
    b0, b1, b2, a1, a2 = design
    z0 = z1 = 0.0
    out = []
    for x in w:
        xc = b0 * x + z0
        z0 = (b1 * x - a1 * xc) + z1
        z1 = b2 * x - a2 * xc
        out.append(limit(xc))
    return out


def run_loop(x, steps):
    """A sox run on a float32 array: steps are designs, or "reverse" """
    w = [limit(float(v)) for v in x]
    for step in steps:
        w = w[::-1] if step == "reverse" else biquad_loop(w, step)
    return np.array(w, dtype=np.float64).astype(np.float32)


def torch_clip(x, factor):
    t = torch.tensor(x, dtype=torch.float32)
    t.clamp_(min=t.min() * factor, max=t.max() * factor)
    return t.numpy()


@pytest.mark.parametrize("name, value", [("low_pass", 3000.0), ("low_pass", 6999.5), ("high_pass", 500.0), ("high_pass", 1987.25),
                                         ("bass", 3.0), ("bass", 20.0), ("bass", 35.0), ("treble", 3.0), ("treble", 19.5)])
def test_each_biquad_is_the_recurrence(name, value):
    x = seeded(300, 1, scale=0.4)
    got = simulate.chain_effects(x, {name: [[True], value]})
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got, run_loop(x, [simulate.biquad_design(name, value)]))


@pytest.mark.parametrize("louder", [1.0, 1.5, 3.7, 10.0, 0.5])
def test_clip_is_torchs_clamp(louder):
    x = seeded(257, 2)
    before = x.copy()
    got = simulate.chain_effects(x, {"clip": [[True], louder]})
    assert got.dtype == np.float32 and np.array_equal(got, torch_clip(x, 1 / louder))
    assert np.array_equal(x, before), "the input is not modified"
    positive = np.abs(x) + np.float32(0.25)      # min and max of one sign
    assert np.array_equal(simulate.chain_effects(positive, {"clip": [[True], louder]}), torch_clip(positive, 1 / louder))


def test_reverse_and_dict_order():
    x = seeded(300, 3, scale=0.7)
    x[10], x[200] = 1.5, -2.0      # a run limits what it takes in, a reverse alone included
    treble, bass, low = (simulate.biquad_design(*p) for p in (("treble", 12.0), ("bass", 6.0), ("low_pass", 4000.0)))
    rev = [True, None]
    assert np.array_equal(simulate.chain_effects(x, {"reverse": rev}), np.clip(x, -1, 1)[::-1])
    assert np.array_equal(simulate.chain_effects(x, {}), x)
    a = simulate.chain_effects(x, {"treble": [[True], 12.0], "reverse": rev, "bass": [[True], 6.0]})
    b = simulate.chain_effects(x, {"treble": [[True], 12.0], "bass": [[True], 6.0], "reverse": rev})
    assert np.array_equal(a, run_loop(x, [treble, "reverse", bass]))
    assert np.array_equal(b, run_loop(x, [treble, bass, "reverse"]))
    assert not np.array_equal(a, b)
    # clip ends a run: the clip is rounded to float32 in front of it and widened again behind it
    c = simulate.chain_effects(x, {"low_pass": [[True], 4000.0], "clip": [[True], 2.0], "reverse": rev, "bass": [[True], 6.0]})
    assert np.array_equal(c, run_loop(torch_clip(run_loop(x, [low]), 0.5), ["reverse", bass]))
    # the type-0 names are the tail's: the chain passes them by, whatever their place in the dict
    d = simulate.chain_effects(x, {"quant": [[True], 4], "bass": [[True], 6.0], "reverb_rir": [True, 0]})
    assert np.array_equal(d, run_loop(x, [bass]))
    # a column is squeezed, any dtype is made float32
    assert np.array_equal(simulate.chain_effects(x[:, None].astype(np.float64), {"bass": [[True], 6.0]}), d)


def test_the_names_that_are_not_built_raise():
    x = seeded(64, 4)
    for name in NOT_BUILT + ("anytime",):
        with pytest.raises(ValueError):
            simulate.chain_effects(x, {"bass": [[True], 6.0], name: [True, [0.1, 0.1, 0.1]]})
    with pytest.raises(ValueError):
        simulate.chain_effects(x, {"flanger": [True, None]})
    with pytest.raises(ValueError):
        simulate.chain_effects(x, {"low_pass": [[True], 22050.0]})


def test_saturation_at_the_sample_range():
    x = (0.5 * np.sin(2 * np.pi * 60 * np.arange(4000) / FS)).astype(np.float32)
    design = simulate.biquad_design("bass", 20.0)
    from scipy.signal import sosfilt
    free = sosfilt(np.array([[design[0], design[1], design[2], 1.0, design[3], design[4]]]), x.astype(np.float64))
    assert 2.8 < np.abs(free).max() < 3.0      # the unlimited peak: 2.89
    y = simulate.chain_effects(x, {"bass": [[True], 20.0]})
    assert y.max() == np.float32(1.0) and y.min() == np.float32(-1.0)
    assert 0.70 < np.mean(np.abs(y) == 1) < 0.75      # 72 % of the samples sit on the limits
    assert np.array_equal(y, run_loop(x, [design]))
    # a treble behind it sees the limited signal, not the unlimited one
    both = simulate.chain_effects(x, {"bass": [[True], 20.0], "treble": [[True], 6.0]})
    treble = simulate.biquad_design("treble", 6.0)
    assert np.array_equal(both, run_loop(x, [design, treble]))
    unlimited = sosfilt(np.array([[treble[0], treble[1], treble[2], 1.0, treble[3], treble[4]]]), free)
    assert not np.array_equal(both, np.clip(unlimited, LO, HI).astype(np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# magical_effects
# ----------------------------------------------------------------------------------------------------------------------
RIRS = [seeded(n, 10 + n, scale=0.2) for n in (40, 75, 120)]


def test_magical_effects_is_the_chain_then_the_tail():
    x = seeded(400, 5, scale=0.3)
    effects = {"low_pass": [[True], 5000.0], "clip": [[True], 2.5], "reverb_rir": [True, 1]}      # the shipped list
    got = simulate.magical_effects(x, effects, RIRS)
    chain = simulate.chain_effects(x, effects)
    want = simulate.array_effects(chain, {"reverb_rir": [True, 1]}, RIRS)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert not np.array_equal(got, chain[:len(got)])
    # dict order: the chain first whatever the place of the type-0 names, the tail in its own order
    mixed = {"quant": [[True], 5], "clip": [[True], 2.5], "reverb_rir": [True, 0], "low_pass": [[True], 5000.0]}
    want = simulate.array_effects(simulate.chain_effects(x, mixed), {"quant": [[True], 5], "reverb_rir": [True, 0]}, RIRS)
    assert np.array_equal(simulate.magical_effects(x, mixed, RIRS), want)
    zeros = simulate.magical_effects(x, {"bass": [[True], 6.0], "empty_c": [True, None]})
    assert zeros.dtype == np.float32 and zeros.shape == x.shape and not zeros.any()
    with pytest.raises(ValueError):
        simulate.magical_effects(x, {"clip": [[True], 2.0], "reverb_rir": [True, 0]})      # no RIRs


def test_largescale_is_decided_on_the_input():
    x = seeded(400, 6, scale=0.3)
    big = (x * np.float32(2 ** 15)).astype(np.float32)      # int16-scaled samples: exact, the largest far above 10
    effects = {"bass": [[True], 20.0], "clip": [[True], 4.0], "reverb_rir": [True, 2]}
    small = simulate.magical_effects(x, effects, RIRS)
    assert np.array_equal(simulate.magical_effects(big, effects, RIRS), small * 2 ** 15)
    ints = big.astype(np.int32)      # any dtype is made float32 first
    assert np.array_equal(simulate.magical_effects(ints, effects, RIRS), simulate.magical_effects(ints.astype(np.float32), effects, RIRS))
    # decided ONCE: samples far beyond 16 bits are still above 10 behind the division and a chain of clip alone (no run limits
    # them); the tail takes them as they are, where `array_effects` on its own would divide again
    huge = (big * np.float32(64)).astype(np.float32)
    got = simulate.magical_effects(huge, {"clip": [[True], 2.0], "quant": [[True], 3]})
    chain = simulate.chain_effects(huge / np.float32(2 ** 15), {"clip": [[True], 2.0]})
    assert chain.max() > 10
    assert np.array_equal(got, simulate.quantification(chain, [[True], 3]) * 2 ** 15)
    before = big.copy()
    simulate.magical_effects(big, effects, RIRS)
    assert np.array_equal(big, before)


@pytest.mark.parametrize("name", NOT_BUILT)
def test_magical_effects_refuses_what_is_not_built(name):
    with pytest.raises(ValueError):
        simulate.magical_effects(seeded(64, 7), {name: [True, [0.1, 0.1, 0.1]], "reverb_rir": [True, 0]}, RIRS)


def test_array_effects_still_refuses_the_chain():
    for name in ("low_pass", "clip", "reverse", "bass", "fade"):
        with pytest.raises(ValueError, match="sox chain"):
            simulate.array_effects(seeded(64, 8), {name: [[True], 2.0]})
        with pytest.raises(ValueError):
            simulate.draw_array_effects(1, P_EFFECTS, [name], 3, np.random.default_rng(0))


# ----------------------------------------------------------------------------------------------------------------------
# draw_effects against a loop that mirrors RandomServer.generate / do
# ----------------------------------------------------------------------------------------------------------------------
def do_mirror(name, p_effects, rir_nums, rng):
    """RandomServer.do(name) with the one NumPy generator in the place of torch.rand"""
    def uniform(lower, upper):
        return upper if abs(lower - upper) < 1e-5 else float((upper - lower) * rng.random() + lower)

    def sample(r):
        assert len(r) == 2
        return float(uniform(r[0], r[1]))

    p = p_effects[name]
    chance = int(rng.random() * 2 ** 31)
    decision = [chance < prob * 2 ** 31 for prob in p["prob"]]
    if not decision[0]:
        return False, None
    if name in ("empty_c", "empty_n", "reverse"):
        return True, None
    if name in ("tempo", "speed"):
        return decision, sample(p["speed_up_range"] if decision[1] else p["speed_down_range"])
    if name == "pitch":
        return decision, sample(p["pitch_up_range"] if decision[1] else p["pitch_down_range"])
    if name in ("treble", "bass", "tremolo"):
        return decision, sample(p["level"])
    if name == "clip":
        return decision, sample(p["louder_time"])
    if name == "low_pass":
        return decision, sample(p["low_pass_range"])
    if name == "high_pass":
        return decision, sample(p["high_pass_range"])
    if name == "reverb_rir":
        return True, int(uniform(0, rir_nums))
    if name == "reverb_freeverb":
        return True, [sample(p["reverb_level"]), sample(p["dumping_factor"]), sample(p["room_size"])]
    if name == "time_dropout":
        start = uniform(p["drop_range"][0], p["drop_range"][1] - p["max_segment"])
        return True, [start, uniform(0.0, p["max_segment"])]
    if name == "quant":
        return decision, int(sample(p["bins"]))
    if name == "fade":
        return True, [sample(p["fade_in_portion"]), sample(p["fade_out_portion"])]
    if name == "anytime":
        return True, [sample(p[k]) for k in ("inner_segment_scale", "overall_scale", "first_segment_portion", "snr_range")]
    raise ValueError("Unknown effect ", name)


def test_draw_effects_mirrors_random_server():
    names = list(P_EFFECTS)
    n = 200      # (treble fires once in twenty)
    got = simulate.draw_effects(n, P_EFFECTS, names, 7, np.random.default_rng(123))
    rng = np.random.default_rng(123)
    want = []
    for _ in range(n):
        item = {}
        for name in names:
            decision, params = do_mirror(name, P_EFFECTS, 7, rng)
            if decision:
                item[name] = [decision, params]
        want.append(item)
    assert got == want and [list(g) for g in got] == [list(w) for w in want]
    for name in names:      # every name was drawn, in both directions where it has two
        assert any(name in g for g in got), name
    for name in ("tempo", "speed", "pitch"):
        assert {g[name][0][1] for g in got if name in g} == {True, False}, name
    # the generator is consumed alike: the next draw agrees
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    simulate.draw_effects(3, P_EFFECTS, names, 7, a)
    for _ in range(3):
        for name in names:
            do_mirror(name, P_EFFECTS, 7, b)
    assert a.random() == b.random()
    # restricted to the type-0 names it is draw_array_effects
    tail = ["reverb_rir", "time_dropout", "quant", "empty_c", "empty_n"]
    assert simulate.draw_effects(20, P_EFFECTS, tail, 7, np.random.default_rng(9)) == \
        simulate.draw_array_effects(20, P_EFFECTS, tail, 7, np.random.default_rng(9))
    with pytest.raises(ValueError):
        simulate.draw_effects(1, P_EFFECTS, ["flanger"], 7, np.random.default_rng(0))


def test_drawn_dicts_run():
    names = ["treble", "bass", "low_pass", "high_pass", "clip", "reverse"]
    x = seeded(200, 11, scale=0.4)
    for effects in simulate.draw_effects(30, P_EFFECTS, names, 0, np.random.default_rng(77)):
        y = simulate.chain_effects(x, effects)
        assert y.dtype == np.float32 and y.shape == x.shape and np.isfinite(y).all()


# ----------------------------------------------------------------------------------------------------------------------
# the list forms on what takes the host path, and the binding
# ----------------------------------------------------------------------------------------------------------------------
def test_list_forms_check_their_arguments_first():
    x = seeded(64, 12)
    with pytest.raises(ValueError):
        simulate.chain_effects_list([x, x], [{}])
    with pytest.raises(ValueError):
        simulate.chain_effects_list([x], [{"tempo": [[True, True], 1.2]}])
    with pytest.raises(ValueError):
        simulate.magical_effects_list([x], [{"fade": [True, [0.1, 0.1]]}])
    with pytest.raises(ValueError):
        simulate.magical_effects_list([x, x], [{}])


def test_effect_chain_supported():
    from voicefixer_main_amd.engine import Engine
    bq = ("biquad", (1.0, 0.0, 0.0, 0.0, 0.0))
    assert Engine.effect_chain_supported([]) and Engine.effect_chain_supported([bq] * 4 + [("clip", 0.5)] + [bq] * 3)
    assert not Engine.effect_chain_supported([bq] * 5)
    assert not Engine.effect_chain_supported([bq, ("reverse",)] * 4 + [bq])      # nine steps
    assert not Engine.effect_chain_supported([bq, bq, ("reverse",), bq, bq, bq])      # a reverse does not end the run
    assert not Engine.effect_chain_supported([("tempo", 1.2)])


def test_chain_kernels_assembly_is_clean(tmp_path):
    """chain.hip on gfx950: no spills, no FLAT memory operations, clean under both assembly checkers"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "chain.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", out, os.path.join(ROOT, "voicefixer_main_amd", "csrc", "chain.hip")],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    kernels = dict(re.findall(r"\n(_ZN3vfx\w+):.*?; ScratchSize: (\d+)", asm, re.S))
    for name in ("k_chain_run", "k_chain_map"):
        assert any(name in k for k in kernels), (name, list(kernels))
    for k, scratch in kernels.items():
        assert int(scratch) == 0, (k, scratch)
    assert not re.search(r"\n\s*flat_(load|store|atomic)", asm)
    assert len(re.findall(r"row_shr:1", asm)) >= 2      # the cascade's hand-over is the DPP move
    for checker in ("asm_store_hazard_check.py", "asm_inflight_check.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", checker), out], capture_output=True, text=True)
        assert r.returncode == 0, (checker, r.stdout[-2000:])


def test_binding_matches_header():
    header = open(os.path.join(ROOT, "include", "vfx.h")).read()
    m = re.search(r"\bint\s+vfx_effect_chain\s*\(([^)]*)\)\s*;", header)
    assert m, "vfx_effect_chain is not declared in include/vfx.h"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib.SIGNATURES["vfx_effect_chain"]
    assert res is _lib.c_int and len(args) == len(params) == 11
    assert [p.split()[-1].lstrip("*") for p in params] == ["h", "x", "B", "ldx", "lengths", "ops", "coef", "K", "y", "ldy", "stream"]
    for want, value in (("VFX_CHAIN_END", 0), ("VFX_CHAIN_BIQUAD", 1), ("VFX_CHAIN_CLIP", 2), ("VFX_CHAIN_REVERSE", 3)):
        assert re.search(r"\b%s = %d\b" % (want, value), header)
    mk = open(os.path.join(ROOT, "voicefixer_main_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bchain\.hip\b", mk, re.M)
