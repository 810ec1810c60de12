"""CPU: the float64 per-piece references of the ResUNet launch tests (tests/resunet_pieces_f64.py) describe the real networks -- the
mel model and, at width 1024 with pruned upsamplers, the spectrogram model --, the cases of tests/test_gpu_resunet_launches.py reach
every split-K factor the planner has, and its spectrogram cases run the network's own shapes and every kernel family of its plan."""
import numpy as np
import torch

import resunet_pieces_f64 as R
from conftest import TOL


def test_piece_references_chain_to_the_oracle(unet_sd):
    """The per-piece references chained in plan order (prep, entry, encoders and pools, bottleneck, decoders, after, final) over
    T = 64, B = 1 reproduce oracle.resunet.generator_mel within the fp32 mode's own bar (the oracle runs in fp32): the references,
    the weight naming and the BatchNorm folding are the network's."""
    from oracle import resunet
    rng = np.random.default_rng(5)
    mel = torch.from_numpy((10.0 ** (rng.normal(size=(1, 64, 128)) * 1.2 - 2.5)).astype(np.float32))
    ref = resunet.generator_mel(unet_sd, mel[:, None])[:, 0].double()
    got = R.generator_mel_chain(unet_sd, mel, p=0)
    assert got.shape == ref.shape == (1, 64, 128)
    d = (got - ref).abs().max().item()
    print("max |chain - oracle| = %.3g" % d)
    assert d < TOL[0]["logmel_max"], d


def test_deep_cases_cover_every_split_k():
    """Host-only: over DEEP_CASES x SHORT_CLIPS the planner picks ksplit 1, 2, 4 and 8, each at least once for a launch with an
    activated output and once for a launch with shortcut segments plus bias -- in both arithmetic modes the ResUNets have."""
    from voicefixer_main_amd.engine import Engine
    for precision in (0, 1, 2):
        act, shortcut = R.splitk_coverage(lambda piece, H, W, sc: Engine.plan_unet_piece(piece, 2, H, W, short_clip=sc, precision=precision))
        assert act >= {1, 2, 4, 8}, (precision, act)
        assert shortcut >= {1, 2, 4, 8}, (precision, shortcut)


def test_spec_piece_references_chain_to_the_oracle():
    """The spectrogram twin of the chain test above: the per-piece references chained at width 1024 with pruned upsamplers (T = 3,
    B = 1: one padded chunk) reproduce oracle.resunet.unet_spec_mag, which runs in fp32, within the fp32 mode's whole-network bar
    relative to the largest magnitude."""
    from oracle import resunet
    from voicefixer_main_amd import synth
    sd = synth.make_resunet_state_dict(2)
    sp = torch.from_numpy(np.abs(np.random.default_rng(6).normal(size=(1, 3, 1025))).astype(np.float32))
    ref = resunet.unet_spec_mag(sd, sp[:, None])[:, 0].double()
    got = R.spec_mag_chain(sd, sp, p=0)
    assert got.shape == ref.shape == (1, 3, 1025) and bool((got[..., 1024] == 0).all())
    d = (got - ref).abs().max().item()
    print("max |chain - oracle| = %.3g, max |oracle| = %.3g" % (d, ref.abs().max().item()))
    assert d < TOL[0]["logmel_max"] * max(1.0, ref.abs().max().item()), d


def test_spec_cases_are_the_networks_shapes():
    """Every spectrogram case of the launch tests runs a piece at a shape the network's own chain gives that piece for T = 64 or 128
    (final and prep: at the trunk's width); level l runs at (Tpad >> (l - 1), 1024 >> (l - 1)), the bottleneck at (1, 16), (2, 16)."""
    import plan_chains as PC
    from voicefixer_main_amd.engine import MODEL_UNET_SPEC
    geometry = {(piece, arg, H, W) for T in (64, 128) for piece, arg, H, W in PC.unet_geometry(MODEL_UNET_SPEC, T)}
    pools = {(H, W, C) for piece, C, H, W in geometry if piece == "pool"}
    cases = R.spec_launch_cases(1)
    for piece, B, H, W, arg, sc, tune in cases:
        if piece == "pool":
            assert (H, W, arg) in pools, (H, W, arg)
        elif piece in ("final", "prep_spec"):
            assert W - (piece == "prep_spec") == PC.UNET_WIDTH[MODEL_UNET_SPEC] and (piece, arg, 64, 1024) in geometry, (piece, arg, W)
        elif piece.endswith(".up") and arg == 0:   # the one odd-width case: the network's input shape, not its pruning
            assert (piece, 1, H, W) in geometry, (piece, H, W)
        else:
            assert (piece, arg, H, W) in geometry, (piece, arg, H, W)
        assert B == (1 if (H, W) == (64, 1024) and piece not in ("pool",) else 2), (piece, B, H, W)
    for l in range(2, 7):
        assert R.SPEC_DEEP_CASES["enc%d.1" % l] == R._level(l, 1024)
    assert R.SPEC_DEEP_CASES["bott"] == [(1, 16), (2, 16)] and R.SPEC_FUSED_SHAPES == [(64, 1024)]
    assert [R.SPEC_UP_CASES[d] for d in range(1, 7)] == [(1 << (d - 1), 16 << (d - 1)) for d in range(1, 7)]
    # every deep piece at both of its level shapes, all three split-K rules
    deep = {(c[0], c[2], c[3], c[5]) for c in cases}
    assert all((piece, H, W, sc) in deep for piece in R.DEEP_CASES for H, W in R.SPEC_DEEP_CASES[piece] for sc in R.SHORT_CLIPS)
    assert all(len(R.SPEC_DEEP_CASES[piece]) == 2 for piece in R.DEEP_CASES)


def _spec_case_families(precision):
    from voicefixer_main_amd import _lib
    from voicefixer_main_amd.engine import Engine
    return {l["family"] for piece, B, H, W, arg, sc, tune in R.spec_launch_cases(precision)
            for l in Engine.plan_unet_piece(piece, B, H, W, arg=arg, short_clip=sc, precision=precision, tuning=getattr(_lib, tune) if tune else 0)}


def test_spec_cases_launch_every_family_of_the_spectrogram_plan():
    """Together the spectrogram cases launch exactly the kernel families the whole spectrogram plan contains, in each arithmetic mode
    (precision 2 runs the ResUNets as precision 1)."""
    from voicefixer_main_amd.engine import Engine, MODEL_UNET_SPEC
    for precision in (0, 1, 2):
        whole = {l["family"] for l in Engine.plan_unet(MODEL_UNET_SPEC, 2, 64, precision=precision)}
        assert _spec_case_families(precision) == whole, (precision, whole)
    assert _spec_case_families(1) == {"small", "k_resblock_in1", "k_block2d32", "k_resblock", "k_resblock_two_src", "k_conv", "k_conv_phased"}


def test_spec_deep_cases_split_k():
    """Host-only twin of test_gpu_resunet_launches.test_spec_deep_cases_split_k: over SPEC_DEEP_CASES x SHORT_CLIPS the planner reaches
    ksplit 1, 2, 4 and 8 -- its whole set, no smaller than the mel cases' -- with an activated output and with shortcut segments plus
    bias, in every arithmetic mode."""
    from voicefixer_main_amd.engine import Engine
    for precision in (0, 1, 2):
        act, shortcut = R.splitk_coverage(lambda piece, H, W, sc: Engine.plan_unet_piece(piece, 2, H, W, short_clip=sc, precision=precision),
                                          R.SPEC_DEEP_CASES)
        assert act == {1, 2, 4, 8} and shortcut == {1, 2, 4, 8}, (precision, act, shortcut)
