"""CPU: the float64 per-piece references of the ResUNet launch tests (tests/resunet_pieces_f64.py) describe the real network, and the
cases of tests/test_gpu_resunet_launches.py reach every split-K factor the planner has."""
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
