"""The case table of tests/test_gpu_large_tensors.py and tests/test_large_tensors_host.py: launches whose largest tensor lies in the
upper half of the 32-bit byte-offset range, (2^31, 2^32 - 4096) bytes.  A plain helper module, no tests.

The convolution families address a tensor with unsigned 32-bit byte offsets from its base (plan.cpp finish_params, resblock.hip
plan_block2d / plan_resblock: a tensor is refused at 2^32 - 4096 bytes), and Engine's calls grow a launch up to that size before they
cut sub-batches -- so signed offset arithmetic, a descriptor's num_records and the reciprocal tile splits at large tile indices are
all live between 2^31 and the limit.  A case is B clips of which clip b holds pattern b mod P: the launch computes every clip alike
(same tiling per image, same split-K factor, deterministic kernels), so clips b >= P must equal clip b - P bit for bit, and clips 0
and 1 are held to the float64 bound their family is held to at small sizes.

`large` is the per-clip shape of the tensor the case is about (4-byte elements unless `ebytes` says otherwise): its byte count and
where byte 2^31 falls in it are arithmetic on this table (Case.nbytes, Case.straddle), never typed in.

The ResUNet's own level shapes are powers of two -- level 1 of the spectrogram model is (64, 1024) x 32 channels = 2^23 bytes a clip
-- so byte 2^31 is the first byte of clip 256 there and no clip straddles it; those cases cover the range, and the *_mel cases
(level 1 and level 3 of the mel model: widths 127 and 31) put the same kernels on clips that do straddle it, inside a tile.  The
vocoder cases take T = 2^15 + 3 positions (the float64 reference of a clip of 2^18 positions takes several seconds of CPU per
convolution; more, shorter clips reach the same bytes): clip 255 (C = 64) / 127 (C = 128) straddles byte 2^31 three positions past a
128-position seam."""
from collections import namedtuple

P = 2                                     # distinct clips of a batch
LO, HI = 1 << 31, (1 << 32) - 4096        # the range a large tensor lies in: above 2 GiB, below what finish_params / plan_resblock refuse
LIMIT16 = 1 << 31                         # resblock_w64.hip launch_resblock_w64, conv_w64.hip conv_w64_ok: the 16-bit families' own limit

_Case = namedtuple("Case", "name kind B large ebytes tiles straddles args")


class Case(_Case):
    @property
    def clip_bytes(self):
        n = self.ebytes
        for d in self.large:
            n *= d
        return n

    @property
    def nbytes(self):
        return self.B * self.clip_bytes

    def straddle(self, at=LO):
        """-> (clip, position, byte within the position) of byte `at` of the tensor; a position is a pixel / a sample (all channels)."""
        pos_bytes = self.large[-1] * self.ebytes
        b, off = divmod(at, self.clip_bytes)
        return (b,) + divmod(off, pos_bytes)


def _case(name, kind, B, large, tiles, straddles=True, ebytes=4, **args):
    return Case(name, kind, B, tuple(large), ebytes, tuple(tiles), straddles, args)


SPEC1 = (64, 1024)     # level 1 of the spectrogram model at Tpad = 64 (resunet_pieces_f64.SPEC_FUSED_SHAPES)
MEL1, MEL3 = (64, 127), (16, 31)   # levels 1 and 3 of the mel model at Tpad = 64 (resunet_pieces_f64._level)

# kind "unet": Engine.op_unet_piece(piece, ...) of `model` ("spec" / "mel") on a handle of `precision`; hw: the piece's input plane; the tile a straddling
# clip is held against is asked of the planner (tests/test_large_tensors_host.py)
UNET_CASES = [
    _case("entry", "unet", 320, SPEC1 + (32,), (), False, piece="entry", model="spec", precision=1, hw=SPEC1, families=["k_resblock_in1"]),
    _case("enc1.2-block2d32", "unet", 320, SPEC1 + (32,), (), False, piece="enc1.2", model="spec", precision=1, hw=SPEC1, families=["k_block2d32"]),
    _case("enc1.2-fp32", "unet", 320, SPEC1 + (32,), (), False, piece="enc1.2", model="spec", precision=0, hw=SPEC1, families=["k_conv", "k_conv"]),
    _case("dec6.1", "unet", 320, SPEC1 + (32,), (), False, piece="dec6.1", model="spec", precision=1, hw=SPEC1, families=["k_resblock_two_src"]),
    _case("after", "unet", 320, SPEC1 + (32,), (), False, piece="after", model="spec", precision=1, hw=SPEC1, families=["k_block2d32"]),
    _case("pool", "unet", 320, SPEC1 + (32,), (), False, piece="pool", model="spec", precision=1, hw=SPEC1, families=["small"]),
    _case("final", "unet", 320, SPEC1 + (32,), (), False, piece="final", model="spec", precision=1, hw=SPEC1, families=["small"]),
    _case("dec6.up", "unet", 320, SPEC1 + (32,), (), False, piece="dec6.up", model="spec", precision=1, hw=(32, 512), families=["k_conv_phased"]),
    _case("enc2.2", "unet", 640, (32, 512, 64), (), False, piece="enc2.2", model="spec", precision=1, hw=(32, 512), families=["k_resblock"]),
    _case("enc3.2", "unet", 1280, (16, 256, 128), (), False, piece="enc3.2", model="spec", precision=1, hw=(16, 256), families=["k_conv", "k_conv"]),
    # the same kernels on clips that straddle byte 2^31 (the mel widths are odd)
    _case("enc1.2-mel", "unet", 2580, MEL1 + (32,), (), piece="enc1.2", model="mel", precision=1, hw=MEL1, families=["k_block2d32"]),
    _case("enc3.2-mel", "unet", 10570, MEL3 + (128,), (), piece="enc3.2", model="mel", precision=1, hw=MEL3, families=["k_conv", "k_conv"]),
]

VT = (1 << 15) + 3     # positions of a vocoder clip
FOLDED = 243           # a dilation set_conv1d_geometry folds into rows of `dil` samples (2 dil + 128 > kPatchMaxRows); 1 is not
# kinds "voc_resblock" (op_voc_resblock: one fused fp32-trunk layer of k_resblock, split-bf16 handle), "voc_conv1d" (op_voc_conv1d,
# 128 -> 128 k3 with a residual: plain k_conv), "voc_upsample" (its output is the large tensor), "voc_final" (its source is);
# tiles: extents in positions the straddling position must be no multiple of -- the 128 positions of a 1-D tile, the row of a folded
# dilation, the 4 x 128 outputs of a phased upsampler tile
VOC_CASES = [
    _case("resblock-c64-d1", "voc_resblock", 320, (VT, 64), (128,), precision=1, C=64, dil=1, fold=0),
    _case("resblock-c64-folded", "voc_resblock", 320, (VT, 64), (128, FOLDED), precision=1, C=64, dil=FOLDED, fold=1),
    _case("resblock-c128-d1", "voc_resblock", 160, (VT, 128), (128,), precision=1, C=128, dil=1, fold=0),
    _case("resblock-c128-folded", "voc_resblock", 160, (VT, 128), (128, FOLDED), precision=1, C=128, dil=FOLDED, fold=1),
    _case("conv1d-d1-fp32", "voc_conv1d", 160, (VT, 128), (128,), precision=0, C=128, dil=1),
    _case("conv1d-folded-fp32", "voc_conv1d", 160, (VT, 128), (128, FOLDED), precision=0, C=128, dil=FOLDED),
    _case("conv1d-d1-bf16", "voc_conv1d", 160, (VT, 128), (128,), precision=1, C=128, dil=1),
    _case("conv1d-folded-bf16", "voc_conv1d", 160, (VT, 128), (128, FOLDED), precision=1, C=128, dil=FOLDED),
    _case("upsample-x4", "voc_upsample", 80, (4 * VT, 64), (128, 512), precision=1, Cin=128, stride=4, T=VT),
    _case("final-c64", "voc_final", 320, (VT, 64), (128,), precision=1, C=64),
]

CASES = UNET_CASES + VOC_CASES


def by_name(name):
    (c,) = [c for c in CASES if c.name == name]
    return c


# Just over a limit the planner refuses on the host, before any launch: (what, piece, B, H, W, precision, the library's error).
# B = the smallest batch whose tensor reaches 2^32 - 4096 bytes at the case's clip size.
def _over(clip_bytes, limit=HI):
    return -(-limit // clip_bytes)


REFUSED_UNET = [
    ("k_block2d32", "enc1.2", _over(1 << 23), SPEC1, 1, "block2d: tensor exceeds 4 GiB"),
    ("k_resblock", "enc2.2", _over(1 << 22), (32, 512), 1, "block2d: tensor exceeds 4 GiB"),
    ("k_conv", "enc3.2", _over(1 << 21), (16, 256), 1, "exceeds 4 GiB"),
    ("k_conv fp32", "enc1.2", _over(1 << 23), SPEC1, 0, "exceeds 4 GiB"),
]
