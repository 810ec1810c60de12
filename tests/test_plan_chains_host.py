"""CPU: the launch list of each whole ResUNet plan is the concatenation of its pieces' lists in the network's order (tests/plan_chains.py).

vfx_plan_unet builds the plan of vfx_resunet_mel / vfx_resunet_spec with build_unet_mel / build_unet_spec on the host;
vfx_plan_unet_piece builds one piece.  Equal lists say that the chain tests/test_gpu_plan_chains.py runs on the GPU is the plan -- not a
different, self-consistent set of launches -- and pin the short_clip class, and with it the split-K factor of every deep convolution,
that a whole call picks from its padded frame count."""
import functools

import pytest

import plan_chains as PC
from voicefixer_main_amd import _lib
from voicefixer_main_amd.engine import MODEL_UNET_MEL, MODEL_UNET_SPEC, Engine

# the frame counts of the GPU tests, plus Tpad 2048 and 4096 (short_clip -2 and -4)
FRAMES = {MODEL_UNET_MEL: (1, 64, 65, 130, 1990, 2048, 4096), MODEL_UNET_SPEC: (3, 70, 130, 2048, 4096)}
CASES = [(m, p, t) for m in (MODEL_UNET_MEL, MODEL_UNET_SPEC) for p in (0, 1) for t in (0,)] + \
        [(MODEL_UNET_MEL, 1, _lib.TUNE_OLD_BLOCK2D), (MODEL_UNET_MEL, 1, _lib.TUNE_TWO_LAUNCH_UPSAMPLERS)]


def _whole(model, B, T, precision, tuning):
    cats = ([], [], [])
    for launch in Engine.plan_unet(model, B, T, precision=precision, tuning=tuning):
        cats[PC.launch_category(launch)].append(launch)
    return cats


def _chain(model, B, T, precision, tuning, **kw):
    return PC.unet_chain_launches(functools.partial(Engine.plan_unet_piece, precision=precision, tuning=tuning), model, B, T, **kw)


def _clips_per_launch(model, T):
    """A whole call runs a batch whose level-1 tensor, cat(up, skip) of 2 x 32 fp32 channels, would pass 4 GiB as consecutive sub-batches
    (the kernels address a tensor with 32-bit byte offsets): the largest batch ONE plan is built for."""
    Tpad = (T + 63) // 64 * 64
    return max(1, (2 ** 32 - 2 ** 20) // (Tpad * PC.UNET_WIDTH[model] * 64 * 4))


def test_short_clip_rule():
    """Tpad <= 128: 1; Tpad >= 2048: -(Tpad / 1024); else 0."""
    assert [PC.short_clip_of(t) for t in (64, 128, 192, 1984, 2048, 3072, 4096)] == [1, 1, 0, 0, -2, -3, -4]


@pytest.mark.parametrize("model,precision,tuning", CASES)
def test_whole_plan_is_the_concatenation_of_its_pieces(model, precision, tuning):
    """Category by category (describe_unet_launches reports a plan's small kernels, then its fused blocks, then its convolutions;
    within a category the order is the launch order): family, ksplit, activated output, bias, K segments and output channels of
    every launch."""
    ksplits = set()
    for T in FRAMES[model]:
        for B in (1, min(16, _clips_per_launch(model, T))):     # (the spectrogram model at Tpad 2048 / 4096: 7 / 3 clips)
            whole, chain = _whole(model, B, T, precision, tuning), _chain(model, B, T, precision, tuning)
            for name, w, c in zip(("small kernels", "fused blocks", "convolutions"), whole, chain):
                assert w == c, (model, precision, tuning, B, T, name, len(w), len(c), [(i, a, b) for i, (a, b) in enumerate(zip(w, c)) if a != b][:4])
            ksplits.update(l["ksplit"] for l in whole[PC.CONVS])
    assert ksplits >= {1, 2, 4, 8}, ksplits      # (the comparison above saw every split-K factor)


def test_the_comparison_sees_a_dropped_piece_and_a_wrong_short_clip():
    """What test_whole_plan_is_the_concatenation_of_its_pieces would miss if it could not fail: without one piece (of any of the three
    categories) the chain's list is another, and so it is with the short_clip of another class wherever the planner splits K."""
    B, T, p = 1, 130, 1
    whole = _whole(MODEL_UNET_MEL, B, T, p, 0)
    steps = PC.unet_steps(MODEL_UNET_MEL)
    assert _chain(MODEL_UNET_MEL, B, T, p, 0) == whole
    for drop in ("pool", "enc1.3", "enc4.2", "dec3.up", "after"):
        i = [s[0] for s in steps].index(drop)
        assert _chain(MODEL_UNET_MEL, B, T, p, 0, steps=steps[:i] + steps[i + 1:]) != whole, drop
    for T, wrong in ((65, 0), (130, 1), (2048, 0)):
        whole = _whole(MODEL_UNET_MEL, B, T, p, 0)
        assert _chain(MODEL_UNET_MEL, B, T, p, 0) == whole
        assert _chain(MODEL_UNET_MEL, B, T, p, 0, short_clip=wrong) != whole, (T, wrong)
