// Internal declarations shared by the libvfx.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "vfx.h"

namespace vfx {

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
struct Error {};  // thrown after set_error(); caught at the C boundary

#define VFX_HIP(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      ::vfx::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      throw ::vfx::Error();                                                                  \
    }                                                                                        \
  } while (0)

#define VFX_CHECK(cond, ...)         \
  do {                               \
    if (!(cond)) {                   \
      ::vfx::set_error(__VA_ARGS__); \
      throw ::vfx::Error();          \
    }                                \
  } while (0)

// The guards of an extern "C" entry point (libvfx.so and libvfx_test.so): nothing is thrown across the C boundary.  An Error is return
// code 1 (its message already set), any other std::exception return code 2 with its what() as vfx_last_error().
#define VFX_API_BEGIN try {
// entry points that take a handle: NULL check + run on the handle's device, restore the caller's on exit
#define VFX_API_BEGIN_H(h) try { VFX_CHECK((h) != nullptr, "NULL handle"); ::vfx::DeviceGuard device_guard_((h)->device);
// ... and launch on a caller's stream: they take turns with calls on other streams of the device (StreamTurn, below)
#define VFX_API_BEGIN_HS(h, stream) VFX_API_BEGIN_H(h) ::vfx::StreamTurn stream_turn_((h)->device, (stream));
#define VFX_API_END                              \
  }                                              \
  catch (const ::vfx::Error&) { return 1; }      \
  catch (const std::exception& e) {              \
    ::vfx::set_error("exception: %s", e.what()); \
    return 2;                                    \
  }                                              \
  return 0;

// Every entry point that takes a handle works on the handle's device whatever the caller's current device is, and
// leaves the caller's current device as it found it (two handles on two GPUs in one process, torch.cuda.set_device
// elsewhere).
struct DeviceGuard {
  int prev = -1, dev = -1;
  explicit DeviceGuard(int device) : dev(device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) VFX_HIP(hipSetDevice(dev));
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Calls on DIFFERENT streams of one device take turns on the GPU timeline: a call first makes its stream wait for the end of the
// previous call of this library on that device and leaves an event behind for the next one.  Why (profiles/r05_two_streams.md,
// profiles/r06_two_streams_xcd.md): with two handles on two streams, k_voc_final -- plain VALU arithmetic -- running while the
// other stream's 16-bit MFMA convolutions of THIS library do (fp16 or split-bf16 operands; not the fp32 MFMA form, not torch's
// hipBLASLt kernels, not any of eight synthetic co-runners; sharing a CU is not required) delivered wrong sums in lanes 48-63 of
// single instructions, a few hundred samples per batch, off by 1e-4 .. 1e-2; every launch is correct when nothing of another
// stream runs beside it.  What is KNOWN: the condition needs this library's hand-scheduled 16-bit convolution kernels on one
// queue and a VALU-dense kernel on another; the same plans on ONE stream, or with a device-wide wait between them, are
// bit-exact.  What is NOT known: the mechanism (an open issue; the aggressors are the kernels with inline-asm loads,
// hand-counted vmcnt and LDS-DMA reads past the buffer bound, so a cause inside this library is not excluded).  Until it is, the
// library does not let its own launches overlap across streams.
//   * The wait is unconditional (an event of the stream's own past is free): no reliance on comparing stream handles, which a
//     destroyed-and-reused stream address would defeat.
//   * A call made while its stream is being CAPTURED into a hipGraph is left alone (an event of another stream cannot enter a
//     capture); a REPLAY of such a graph is not a call of this library -- callers bracket it with vfx_turn_begin / vfx_turn_end
//     (include/vfx.h; Engine.replay) or keep replays on the one stream everything else uses.
//   * Host threads: the mutex is held for the duration of a call (the next call's wait needs this call's end event, which exists
//     only once the call is enqueued), so calls on one device are ENQUEUED one at a time, plan builds included.  Handles are
//     not thread-safe anyway; multi-threaded callers serialise on this lock per device.
//   * Other PROCESSES on the same GPU are outside this guard -- and round 6 measured that a second process running this library's
//     ResUNet disturbs this process's k_voc_final just the same (every batch wrong, RAS counters silent): one process per GPU
//     (dist.py) is the supported deployment.
// VFX_NO_STREAM_TURNS=1 in the environment switches the turns off (scripts/two_streams_xcd.py needs the overlap it measures).
struct DeviceTurn {
  std::mutex mu;
  hipEvent_t done = nullptr;   // end of the last call on this device
  bool any = false;
};
DeviceTurn& device_turn(int device);  // api.cpp
bool stream_turns_enabled();          // api.cpp
// the two halves, also exported as vfx_turn_begin / vfx_turn_end (each takes the lock for its own bookkeeping only)
inline void turn_wait(DeviceTurn& d, hipStream_t s) {
  if (d.any) VFX_HIP(hipStreamWaitEvent(s, d.done, 0));
}
inline bool turn_record(DeviceTurn& d, hipStream_t s) {
  if (!d.done && hipEventCreateWithFlags(&d.done, hipEventDisableTiming) != hipSuccess) return false;
  if (hipEventRecord(d.done, s) != hipSuccess) return false;
  d.any = true;
  return true;
}
struct StreamTurn {
  DeviceTurn& d;
  std::unique_lock<std::mutex> lock;
  hipStream_t s;
  bool active = false;
  StreamTurn(int device, void* stream) : d(device_turn(device)), lock(d.mu), s(static_cast<hipStream_t>(stream)) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
      (void)hipGetLastError();
      cs = hipStreamCaptureStatusNone;
    }
    active = cs == hipStreamCaptureStatusNone && stream_turns_enabled();
    if (active) turn_wait(d, s);
  }
  ~StreamTurn() {
    if (active) (void)turn_record(d, s);
  }
  StreamTurn(const StreamTurn&) = delete;
  StreamTurn& operator=(const StreamTurn&) = delete;
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device property of a kernel: done once per (kernel, device).
inline bool first_use_on_current_device(uint64_t& mask) {
  int dev = 0;
  VFX_HIP(hipGetDevice(&dev));
  const uint64_t bit = uint64_t(1) << (dev & 63);
  if (mask & bit) return false;
  mask |= bit;
  return true;
}

// ---------------------------------------------------------------------------------------------
// stage-driven tap-convolution (implicit GEMM on the MFMA) -- see conv.hip
// ---------------------------------------------------------------------------------------------
constexpr int kMaxTaps = 9;
constexpr int kMaxSegs = 3;
constexpr int kKC = 32;             // input channels per K step
constexpr int kIdentityLen = 4096;  // length of the identity scale/shift tables
constexpr int kPatchMaxRows = 192;
constexpr int kMaxVarlenClips = 1024;  // clips per launch of a varlen batch (vfx_handle::d_lens)
// The rows of vfx_handle::d_lens, kMaxVarlenClips ints each: per-clip lengths of the call in flight, written in stream order behind the
// kernels of the previous call.  launch_set_lens fills three consecutive rows at once (which is why row 5 exists: nobody reads it).
enum LensRow {
  LENS_SAMPLES = 0, LENS_FRAMES = 1, LENS_VOC_FRAMES = 2,              // samples / frames / vocoder frames of the varlen batch
  LENS_GROUP_FRAMES = 3, LENS_GROUP_INDEX = 4,                         // frames / batch index of the clips of its ResUNet group in flight
  LENS_RUN_SAMPLES = 6, LENS_RUN_FRAMES = 7, LENS_RUN_VOC_FRAMES = 8,  // samples / frames / vocoder frames of its vocoder run in flight
  LENS_ANALYSIS_FRAMES = 9,                                            // frames per clip of a vfx_analysis_mel call
  LENS_SCORE_SAMPLES = 10, LENS_SCORE_FRAMES = 11,                     // samples / frames of the vfx_audio_metrics sub-batch in flight
  LENS_LOWPASS_SAMPLES = 12, LENS_LOWPASS_CUT = 13,                    // samples / cut-off bin of the vfx_stft_lowpass sub-batch in flight
  LENS_STOI_SAMPLES = 14, LENS_STOI_OUT = 15, LENS_STOI_FRAMES = 16,   // input samples / 10 kHz samples / frames of the vfx_stoi sub-batch in flight
  LENS_TARGET_SAMPLES = 17,                                            // samples of the targets of a vfx_restore_*_varlen_scored call
  LENS_BSS_SAMPLES = 18,                                               // samples of the vfx_bsseval sub-batch in flight
  LENS_LOSS_COUNT = 19, LENS_LOSS_FRAMES = 20,                         // elements per row / frames of the vfx_spec_losses or vfx_validate_gsr_varlen sub-batch in flight
  LENS_SPLICE_SAMPLES = 21, LENS_SPLICE_CUT = 22, LENS_SPLICE_GAIN = 23,  // samples / cut-off bin / gain (a float32 bit pattern) of the vfx_stft_splice sub-batch in flight
  LENS_POWER_SAMPLES = 24, LENS_POWER_FRAMES = 25,                     // samples / frames of the vfx_band_power sub-batch in flight ...
  LENS_POWER_LO = 26, LENS_POWER_HI = 27,                              // ... and the first bin of its band / the bin behind it
  kLensRows = 28
};
constexpr size_t kMaxCachedPlans = 32; // per handle (round 5: 8 -> 32 -- a file with a target alternates between more than eight (stage, B, T) keys and rebuilt plans on every call; a plan is ~0.4 MB on each side); a plan owns host + device parameter blocks (the eval handler's last
                                        // segment has a new length for every file)  // patch pixels per stage (6 row groups of 32)

enum Act { ACT_NONE = 0, ACT_LEAKY = 1, ACT_ELU = 2 };

// One K-range of the implicit GEMM: a source tensor (channels-last), its prologue
// (per-channel affine + activation, applied while the patch is staged into LDS; positions
// outside the tensor are 0 AFTER the prologue) and a tap list with K-chunked weights.
struct TapSeg {
  const float* src;    // (B, Hi, Wi, C)
  const float* scale;  // [C] or nullptr (=1)
  const float* shift;  // [C] or nullptr (=0)
  const float* wt;     // fragment-packed [C/32][ntaps][Cout/32][1024] (pack_conv)
  int C;
  int ntaps;
  int act;
  float slope;
  int src_act;         // 1: src is an ACTIVATED tensor (see TapConvParams::out_act): staged by plain copy, no prologue
  int dh[kMaxTaps];
  int dw[kMaxTaps];
};

// One stage of a launch: a 32-channel chunk of one source and the taps that read it through one
// staged patch.  Read by the kernel with scalar loads; built by build_stages() at bind time.
struct ConvStage {
  const float* src;    // source tensor + channel offset of the chunk
  const float* scale;  // prologue affine of the chunk's 32 channels
  const float* shift;
  const float* wt;     // weights of the stage's first tap, cout block 0
  int C;               // pixel stride of src in floats
  int dh0, dw0;        // patch origin relative to the tile origin
  int ntaps;
  float slope;         // LeakyReLU slope of the prologue (1 = identity, 0 = ReLU)
  int tap_stride;      // floats between the weights of consecutive taps (Cout * 32)
  int flags;           // bit 0: src is an activated tensor (LDS-DMA copy, no prologue)
  unsigned nbytes;     // bytes addressable from src (buffer descriptor bound; reads past it return 0)
  int poff[16];        // per tap (kMaxTaps used): patch row offset | column shift << 16 | row shift << 24
};
static_assert(sizeof(ConvStage) == 128, "ConvStage is read as a 128-byte record");

// Tile geometry of a k_conv_w64 launch (plan_conv_w64): 128 outputs per tile -- a 1-D run for dilations up to 16 (patch: 128 + 2 dil
// rows), above that 8 rows x 16 columns of the sequence folded into rows of `dil` samples (patch: 10 x 16 rows; the taps are vertical).
struct ConvW64Geo {
  int want;         // the plan asks for the kernel (voc_conv1d_params); add_conv clears it when the launch does not fit
  int on;           // the launch runs on k_conv_w64
  int fold;
  int T, dil;       // positions per clip (the stride between clips), dilation
  int tiles_h, tiles_w;
  int P;            // patch rows in use (<= 160)
  int poff[3];      // patch row offset of the taps
  unsigned long long inv_tiles_w, inv_tiles_per_img;  // ceil(2^32 / n): div_recip() (conv_common.h)
};

struct TapConvParams {
  TapSeg seg[kMaxSegs];
  int nseg;
  int total_steps;       // sum over segs of ntaps * C/32
  int B, Hi, Wi;         // input spatial extent (shared by all segments)
  int Hg, Wg;            // logical grid: one GEMM row per (b, i < Hg, j < Wg)
  int Ho, Wo, Cout;      // output tensor (B, Ho, Wo, Cout)
  int sh, sw, oh0, ow0;  // grid (i, j) -> output pixel (i*sh + oh0, j*sw + ow0), masked to Ho x Wo
  int reflect_w;         // reflect addressing along W (ReflectionPad1d) instead of zero padding
  // Folded 1-D geometry (Conv1d with dilation d viewed as a 2-D convolution with VERTICAL taps on the
  // sequence reshaped to rows of d samples): pixel (i, j) of image b is element b * img_stride + i * W + j
  // and exists iff i * W + j < limit.  0 = plain 2-D tensors (img_stride = limit = H * W); set by finish_params.
  int in_img_stride, in_limit;
  int out_img_stride, out_limit;
  int M;                 // output pixels of the launch (B * Hg * Wg, or B * out_limit when folded)
  int split;             // 1 = split-bf16 operand mode, 0 = exact fp32
  int hionly;            // 16-bit operands: split layouts, but the hi halves hold fp16 values and are the only ones
                         // loaded and multiplied (1 MFMA per product); weights packed with mode 2
  // tile / patch geometry (plan_conv): the M tile is a TH x TW block of the logical grid of one image,
  // every stage stages a PH x PW patch (P = PH * PW <= kPatchMaxRows pixels).
  int TH, TW, tw_shift;   // TH * TW <= 128, TW = 1 << tw_shift
  int tiles_h, tiles_w;   // tiles per image
  int PW, P;
  int per_tap;            // 1: the taps are too far apart for one patch -> one stage per (chunk, tap)
  int dh_min, dw_min;     // patch origin of the all-taps window
  int nstages;
  const ConvStage* stages;  // device table (bind time)
  // Phased launch (the output phases of a transposed convolution as ONE launch): Cout = nphase * cout_phase, the
  // couts [r * cout_phase, (r+1) * cout_phase) are phase r with its own stage table (stages + r * nstages) and its own
  // weight tensor.  With the output viewed as (B, T, nphase * cout_phase) this IS ConvTranspose1d's (B, T * nphase,
  // cout_phase): the input patch is fetched from HBM once for all phases.  nphase = 0 / 1: ordinary launch.
  int nphase, cout_phase;
  // Phased launch onto an ODD output width (round 4: the mel ResUNet's upsamplers, output width 2 W + 1): the two column classes
  // of one output row class cannot be viewed as channel halves of a (B, H, W', 2 C) tensor -- rows of 2 W + 1 pixels do not split
  // into pairs -- so the output is addressed in units of out_cmul = C channels: pixel index (oh * Wo + 2 j) of the TRUE tensor,
  // phase r at channel offset r * C, i.e. at true column 2 j + r; phase 1 has one column fewer (masked: ow + r < Wo).
  // 0 = ordinary addressing (pixel index * Cout).  No residual, activated output or split-K with it.
  int out_cmul;
  // Round 6: BOTH output row classes of such an upsampler in one launch -- four phases r = 2 a + b, phase r writes output row
  // 2 i + a (oh0 = 0, sh = 2) and true column 2 j + b; the four blocks of a spatial tile are neighbours in the tile order and share one
  // patch through their XCD's L2: x is read from HBM once instead of twice, one launch instead of two.  Needs out_cmul.
  int phase_rows;
  double flops_override;  // algorithmic flops when they are not 2 * M * Cout * K (phased launches)
  const float* bias;     // [Cout] or nullptr
  const float* residual; // (B, Ho, Wo, Cout) or nullptr, added in the epilogue
  // 16-bit mode, fp16 trunk (round 4): the residual as the ACTIVATED fp16 tensor fp16(LeakyReLU(r, slope)) that the launch's
  // producer chain already stores for a convolution -- the raw value is recovered as min(v, v * residual_inv_slope) (LeakyReLU
  // with a positive slope is invertible; cf. ResBlockParams::x16), so a two-launch ResStack layer keeps NO raw tensor at all.
  const float* residual_act;
  float residual_inv_slope;
  float* out;            // raw fp32 output (B, Ho, Wo, Cout) or nullptr
  // Optional ACTIVATED output for a tensor whose only consumer is the next convolution: the epilogue
  // applies that consumer's prologue (per-channel affine, LeakyReLU / ELU) once per element and stores
  // the MFMA operand form: per pixel and 32-channel chunk [32 hi bf16 | 32 lo bf16] in split-bf16 mode and 32
  // activated floats in fp32 mode (same size as fp32); in the 16-bit mode (hionly) an fp16 tensor, 2 bytes per
  // element, channels in natural order.  The consumer stages it by plain copy (LDS-DMA).
  float* out_act;
  const float* act_scale;  // [Cout] or nullptr (=1)
  const float* act_shift;  // [Cout] or nullptr (=0)
  float act_slope;         // LeakyReLU slope in [0, 1] (1 = identity)
  int act_elu;             // 1: ELU instead of LeakyReLU
  int* flags;              // the handle's sticky device flags (VFX_FLAG_F16_SATURATED); may be NULL
  // Split-K (choose_ksplit): the deep ResUNet levels have a few hundred output pixels per clip and K = 3456 .. 6912 -- a
  // launch of 100 .. 400 blocks that each walk the whole K range.  ksplit > 1: the stage table is cut into ksplit
  // consecutive ranges, block (tile, s) accumulates range s and stores its raw fp32 partial tile into slice s of `ws`
  // ([ksplit][B * out_img_stride][Cout]); k_splitk_reduce adds the slices in order and applies the epilogue (bias,
  // residual, raw / activated output).  The split depends on the per-clip geometry only, never on the batch size:
  // results do not depend on how clips are batched.
  int ksplit;
  // Set by the plan (PlanBuilder::short_clip): the clip has at most 128 padded frames (the 1-s streaming chunk).  Such a clip
  // cannot fill the chip whatever the batch is asked to be -- the deep launches are pure latency chains -- so the split aims at
  // 512 blocks per clip with slices of one stage (round 4: 3.16 -> 2.51 ms per 1-s chunk; the same rule costs a 16 x 10 s batch
  // +20 %, profiles/r04_c8_splitk_ab.txt).  A property of the CLIP, never of the batch: results stay batch-invariant.
  int short_clip;        // (< 0: a LONG clip of -short_clip x 1024 padded frames -- the split aims at 128 x that many blocks per clip)
  float* ws;
  int tuning;            // vfx_config.tuning of the handle (choose_ksplit)
  // Batches of clips of unequal length (vfx_restore_gsr_varlen; 1-D launches of the vocoder): lens[b] = length of clip b in
  // vocoder frames (T_b + T_b % 2 + 4), a device array owned by the handle and refilled by every call; the clip's input /
  // output sequence ends at lens[b] * lens_mul_in / lens_mul_out positions (the launch's own units: a phased upsampler
  // addresses its output in INPUT positions).  NULL = every clip has the full length (all other launches).  No split-K with it.
  const int* lens;
  int lens_mul_in, lens_mul_out;
  // Set by PlanBuilder::add_conv_phased: this phased launch (a ConvTranspose1d of the vocoder's 16-bit mode: activated fp16 source,
  // one fp16 output) runs on k_up16 (upsample16.hip) -- one block per tile of input positions and ALL its output phases, the patch
  // staged once -- instead of k_conv's block per (tile, phase, cout range).  Same stage tables, same sums.
  int up16;
  // Set by voc_conv1d_params / PlanBuilder::add_conv: this launch (a convolution of a two-launch ResStack layer of the vocoder's 16-bit
  // mode: k3, activated fp16 source, one activated fp16 output, the residual -- if any -- in activated form) runs on k_conv_w64
  // (conv_w64.hip: four-wave blocks of 64-cout waves, two per CU, the patch as a ring of four chunk buffers) with the tile geometry
  // below instead of the one above.  Same weights, same summation order, same bits.
  ConvW64Geo w64;
};

// One fused TFGAN ResStack layer (resblock.hip): y = x + conv2(LeakyReLU(conv1(LeakyReLU(x)) + b1)) + b2.
struct ResBlockParams {
  const float* x;   // (B, T, C) raw fp32 input, also the residual
  float* y;         // (B, T, C) raw fp32 output
  const float* w1;  // conv1 (k3, dilation dil), fragment-packed [C/32][3][C/32][1024] (pack_conv)
  const float* w2;  // conv2 (k3, dilation 1)
  const float* b1;  // [C]
  const float* b2;
  float slope;      // LeakyReLU slope of both activations
  int B, T, C, dil;
  // tile geometry (plan_resblock): h tile = TH x W1 positions, position(li, lj) = base + li * rowstride + lj
  int fold;         // 1: the sequence is viewed as rows of `dil` samples (conv1's taps are vertical)
  int TH, W1, TWo;  // TWo = outputs per tile row (W1 - 2)
  int tiles_h, tiles_w;
  int PW, P;        // x patch: PH x PW pixels, P <= kPatchMaxRows
  int poff[3];      // patch row offset of conv1's taps
  int hionly;       // fp16 operands in the hi halves only, cf. TapConvParams::hionly
  int* flags;       // the handle's sticky device flags (VFX_FLAG_F16_SATURATED); may be NULL
  // Wide stacks of the 16-bit mode (resblock_w64.hip, C = 256): conv1 reads the activated fp16 tensor
  // xa = fp16(LeakyReLU(x)) (2 bytes per element) through the LDS-DMA engine, no arithmetic on it; besides y the kernel
  // writes ya = fp16(LeakyReLU(y, act_slope)) for the next consumer (NULL: not needed).  Weights: pack_conv mode 3.
  //   x16 == 0 (VFX_TUNE_F32_TRUNK): two-form trunk -- x is the raw fp32 residual, y the raw fp32 output (12 bytes per element);
  //   x16 == 1: the activated fp16 tensor is the ONLY form of the trunk (4 bytes per element): x and y are NULL, the residual
  //   is recovered from xa (LeakyReLU with a positive slope is invertible: x = xa >= 0 ? xa : xa / slope -- the same relative
  //   precision as fp16(x)), ya must be there.
  int asrc;
  // fp16 residual trunk of the 16-bit mode (the default; VFX_TUNE_F32_TRUNK = 0 here): x and y point to fp16 tensors (B, T, C),
  // 2 bytes per element, channels in natural order.  The layer's arithmetic is unchanged -- fp16 operands, fp32 accumulation,
  // the residual added in fp32 in registers -- only what travels between two launches is rounded (saturation is flagged).
  // y may be NULL when only ya is consumed (the last layer of a stack in front of an upsampler).
  int x16;
  int tile_m;       // h positions per tile: 0 = 128 (k_resblock, resblock_w64, resblock_r128); resblock_rw: 256
  // Layer pair (resblock_rw.hip, PAIR): dil2 > 0 = a second layer (dilation dil2, weights w1b .. b2b, same slope) follows in the
  // same launch; y is ITS output, the first layer's output is never stored.
  int dil2;
  const float* w1b;
  const float* w2b;
  const float* b1b;
  const float* b2b;
  int r128;         // set by plan_resblock: resblock_r128.hip runs this layer (16-bit mode, C = 128)
  int rw;           // set by plan_resblock: the persistent register-weights kernel runs this layer (resblock_rw.hip: 16-bit mode, C = 64)
  const float* xa;
  float* ya;
  float act_slope;
  // 2-D ConvBlockRes mode (plan_block2d): x, y are (B, H, W, C), both convolutions 3x3, folded BatchNorm affines
  int geo2d, H, W;
  const float* sc1;  // bn1 scale / shift [C]: prologue of conv1
  const float* sh1;
  const float* sc2;  // bn2 scale / shift [C]: prologue of conv2, applied to h
  const float* sh2;
  // entry block (k_resblock<.., IN1>): x is the single-channel input plane (B, H, W), w1 the [tap][32] conv1 weights, bn1 the
  // scalar affine below, wsc / bsc the 1x1 shortcut (weight and bias per output channel); sc1 / sh1 are unused
  int in1;
  float in1_scale, in1_shift;
  const float* wsc;
  const float* bsc;
  // two-source block (k_resblock<.., SC2>; decoder level 1): the input is cat(x, x2) (C channels each), w1 / w1x2 the conv1 weights
  // of the two sources, sc1 / sh1 hold 2 C channels, wsc / wsc2 the fragment-packed 1x1 shortcut of each source, bsc its bias
  int two_src;
  const float* x2;
  const float* w1x2;
  const float* wsc2;
  int poff9[9];      // conv1: patch row offset of tap (dy, dx)
  int hoff9[9];      // conv2: h row offset of tap (dy, dx)
  // set by plan_resblock: multiply-shift reciprocals, n / d = (n * inv) >> 20 (exact for n < 512, d <= 320), and the tile ->
  // (image, tile row, tile column) split as (tile * inv_tpi) >> 32 etc. (exact for tile < 2^32 / d)
  unsigned inv_pw, inv_w1;
  // ceil(2^32 / n) for n = tiles_w, tiles_w * tiles_h: 33 bits when n = 1 (one tile per image: short sequences) -- div_recip()
  unsigned long long inv_tiles_w, inv_tiles_per_img;
  int recip_ok;      // plan_block2d: the reciprocal tile split is exact for this launch's tile count
  int patch_rows;    // set by plan_resblock: rows of a patch buffer when they are not tile_m + 64 (resblock_w64.hip: 160)
  int tuning;        // vfx_config.tuning of the handle: which kernel family runs the layer (plan_resblock)
  // Batches of clips of unequal length (cf. TapConvParams::lens): clip b's sequence ends at lens[b] * lens_mul positions; T stays
  // the stride between clips.  NULL = T for every clip.  1-D layers only.
  const int* lens;
  int lens_mul;
  // Timing builds only (-DVFX_TIMING, scripts/phase_timing.py): [tile][wave][16] s_memtime stamps of the 4-wave kernels' phases
  unsigned long long* timing;
};
bool resblock_supported(int C);
int resblock_block_waves(const ResBlockParams& hp);
// resblock_rw.hip: C = 64, 16-bit mode -- persistent blocks, weights in registers, next patch prefetched into registers
// resblock_w64.hip: the wide layer (C = 256, 16-bit mode) as 4-wave blocks of 64-cout waves, two blocks per CU
bool resblock_w64_supported(int C);
// resblock_r128.hip: C = 128, 16-bit mode -- 4-wave blocks, two per CU, x read once (the residual stays in registers)
bool resblock_r128_pair_ok(int C, int dil, int dil2, int tuning);  // two layers (dil, dil2) as one launch: (1, 3)
int resblock_r128_patch_rows();
void launch_resblock_r128(const ResBlockParams& hp, const ResBlockParams* dparams, hipStream_t stream);
int resblock_w64_patch_rows();
void launch_resblock_w64(const ResBlockParams& hp, const ResBlockParams* dparams, hipStream_t stream);
int resblock_rw_tile(int tuning);
bool resblock_rw_pair_ok(int C, int dil, int dil2, int tuning);  // this pair of consecutive layers can run as one launch
void launch_resblock_rw(const ResBlockParams& hp, const ResBlockParams* dparams, hipStream_t stream);
// compute units of the current device (cached per device): grid size of the persistent kernels
int cu_count_of_current_device();
bool block2d_supported(int C);
void plan_resblock(ResBlockParams& p);
void plan_block2d(ResBlockParams& p);
void launch_resblock(const ResBlockParams& hp, const ResBlockParams* dparams, hipStream_t stream);
double resblock_flops(const ResBlockParams& hp);

// Geometry + taps of a Conv1d (kernel K, dilation dil, 'same' padding) over (B, T, C) tensors as seg[0] of p:
// plain 1-D when the taps fit one patch, folded (rows of `dil` samples, vertical taps) otherwise.
void set_conv1d_geometry(TapConvParams& p, int B, int T, int K, int dil, bool reflect);
void finish_params(TapConvParams& p);  // fills total_steps, M and the tile / patch geometry, validates
int count_stages(const TapConvParams& p);
int choose_ksplit(const TapConvParams& p);  // after finish_params
void launch_splitk_reduce(const TapConvParams& hp, hipStream_t stream);  // hp: absolute pointers
void build_stages(const TapConvParams& p, const float* ones, const float* zeros, ConvStage* out);  // p: absolute pointers
void launch_conv(const TapConvParams& hp, const TapConvParams* dparams, hipStream_t stream);
int conv_block_n(const TapConvParams& hp);
bool block2d32_ok(const ResBlockParams& hp);  // block2d32.hip
bool block2d32_has_tile(int TH, int W1);
void launch_block2d32(const ResBlockParams& hp, const ResBlockParams* dparams, hipStream_t stream);
bool upsample16_ok(const TapConvParams& hp);  // upsample16.hip
// conv_w64.hip: hp (after finish_params) is a launch k_conv_w64 runs; plan_conv_w64 fills hp.w64 for it
bool conv_w64_ok(const TapConvParams& hp);
void plan_conv_w64(TapConvParams& hp);
void launch_conv_w64(const TapConvParams& hp, const TapConvParams* dparams, hipStream_t stream);
void launch_upsample16(const TapConvParams& hp, const TapConvParams* dparams, hipStream_t stream);
double conv_flops(const TapConvParams& hp);

// ---------------------------------------------------------------------------------------------
// front-end tables + small kernels -- see stft.hip / small_ops.hip
// ---------------------------------------------------------------------------------------------
constexpr int kMelNnzMax = 2048;  // non-zeros of the mel filterbank that k_stft_mel keeps in LDS (2018 for the 128-band HTK table)

struct FrontEndTables {
  float* window = nullptr;    // [2048] periodic Hann
  float* twiddle = nullptr;   // [1024] float2 e^{-2 pi i m / 1024}
  float* rtwiddle = nullptr;  // [1025] float2 e^{-2 pi i k / 2048}
  float* fb_val = nullptr;    // packed non-zeros of the mel filterbank, band-major
  int* fb_start = nullptr;    // [128] first frequency bin of band m
  int* fb_off = nullptr;      // [129] offsets into fb_val
  int fb_nnz = 0;             // entries of fb_val (<= kMelNnzMax: k_stft_mel keeps them in LDS)
  float* voc_inv_weight = nullptr;  // [128] 1 / mel band weight
};

// lens != nullptr (device, [B]): clip b holds lens[b] <= L samples in its row of L (batches of clips of unequal length)
void launch_stft_mel(const FrontEndTables& t, const float* wav, int B, int L, int T, float* mel, float* sp,
                     float* cosp, float* sinp, int log10_mel, int hop, float eps, hipStream_t stream,
                     const int* lens = nullptr);
void launch_mel_project(const FrontEndTables& t, const float* sp, int64_t rows, float* mel, hipStream_t stream);
void launch_istft(const FrontEndTables& t, const float* re, const float* im, int B, int T, int L, int hop, float* wav,
                  hipStream_t stream, const int* lens = nullptr);  // lens: samples per clip of a varlen batch (device, [B])
// STFT -> zero the bins k >= cut[b] -> ISTFT in one launch: wav (B, L), clip b = its first lens[b] samples (n_fft/2 < lens[b] <= L),
// -> out (B, L), zeros past lens[b]; lens, cut: device, [B].  out must not overlap wav.  Bit for bit launch_stft_mel's sp * cos and
// sp * sin, masked, through launch_istft.
void launch_stft_lowpass(const FrontEndTables& t, const float* wav, int B, int L, int hop, const int* lens, const int* cut,
                         float* out, hipStream_t stream);
// The splice in one launch: x, y (B, L), pair b = the first lens[b] samples of both rows -> out (B, L) = g y + ISTFT(a . STFT(x - g y)),
// g = gains[b] (float32 bit patterns), a = 1 below bin cut[b] - ramp, the linear ramp (cut[b] - k) / (ramp + 1) up to cut[b], 0 from
// there; zeros past lens[b]; lens, cut, gains: device, [B].  out must overlap neither x nor y.  Bit for bit launch_stft_mel of
// d = x - g y, its sp * cos and sp * sin weighted, through launch_istft, plus g y.
void launch_stft_splice(const FrontEndTables& t, const float* x, const float* y, int B, int L, int hop, const int* lens, const int* cut,
                        const int* gains, int ramp, float* out, hipStream_t stream);
// The launch geometry of these (host-only; the tests assert the geometry they exercise through these): the frames a wave of
// k_stft_mel walks for a launch of `frames` = B * T frames; the hops a workgroup of k_istft / k_stft_lowpass / k_stft_splice owns and
// the groups per clip
int frames_per_group(int64_t frames);
struct IstftGrid {
  int IH, span, groups;
};
IstftGrid istft_grid(int B, int T, int L, int hop);

void launch_prep_logmel(const float* mel_linear, int B, int T, int Tpad, float* x, int* flags, hipStream_t s,
                        const int* lens_t = nullptr);  // lens_t: frames per clip of a varlen batch (device, [B])
void launch_prep_spec(const float* sp, int B, int T, int Tpad, float* x, hipStream_t s, const int* lens_t = nullptr);
void launch_conv_c1(const float* x, int B, int H, int W, const float* w9x32, float scale, float shift, float slope,
                    const float* wsc32, const float* bsc32, float* h, float* sc, hipStream_t s);
void launch_avgpool2(const float* x, int B, int H, int W, int C, float* y, hipStream_t s);
void launch_final_1x1(const float* y, int B, int Tpad, int W, const float* w32, float bias, int mode, int T,
                      const float* aux0, const float* aux1, float* out0, float* out1, hipStream_t s);
void launch_voc_prep(const float* mel, int B, int T, int Tp, const float* inv_weight, float amp_floor, float min_db,
                     float range, float* cond, hipStream_t s, const int* lens_t = nullptr);
// x_f16: x is an fp16 tensor (the fp16 trunk of the 16-bit mode); lens: vocoder frames per clip of a varlen batch, hop samples each
void launch_voc_final(const float* x, int x_f16, int B, int T, int C, const float* w, float bias, float slope, float* wav,
                      unsigned* peak, hipStream_t s, const int* lens = nullptr, int hop = 1);
// d_lens[r * cap + b] = host[r * B + b], r < 3 (samples, frames, vocoder frames per clip): as kernel arguments, in stream order
void launch_set_lens(int* d_lens, int cap, const int* host, int B, hipStream_t s);
void launch_copy_rows_masked(const float* src, float* dst, int B, int T, int F, const int* lens_t, hipStream_t s);
// dst (n, Tg, F) compact <- rows of src (B, T, F) of the clips idx[j] (rows >= T: zeros);  ... and back (rows < min(T, Tg))
void launch_gather_rows(const float* src, const int* idx, float* dst, int n, int T, int Tg, int F, hipStream_t s);
void launch_scatter_rows(const float* src, const int* idx, float* dst, int n, int T, int Tg, int F, hipStream_t s);
void launch_peak_trim_varlen(const float* wav_long, int B, int64_t Llong, int L, int hop, const int* lens_l, const int* lens_tp,
                             const float* peak, float* out, hipStream_t s, int* flags);
void launch_from_log(const float* logmel, const float* mel_in, int B, int T, int unify, float* sums, float* mel_out,
                     hipStream_t s, const int* lens_t = nullptr);
// from_log of one value (pytorch_util.py:161-163): the one expression behind k_from_log and the handler scores of score.hip
__device__ __forceinline__ float from_log_value(float logmel) { return exp10f(fminf(logmel, 5.f)); }
// peak (device, [B]): each clip's peak as the vocoder tail left it; flags: VFX_FLAG_PEAK_NORMALISED when a clip was divided by its peak
void launch_peak_trim(const float* wav_long, int B, int64_t Llong, int L, const float* peak, float* out, hipStream_t s,
                      int* flags = nullptr);
void launch_spectral_metrics(const float* est, const float* tgt, int B, int T, int F, double* ws, float* out, hipStream_t s);

// score.hip: the scores of vfx_audio_metrics.  Per-clip partial sums (float64) in ws; lens = samples, frames = rows per clip (device)
constexpr int kSisdrSlab = 16384;                    // samples per partial sum of the SI-SDR inner products
constexpr int kSsimTileH = 32, kSsimTileW = 64;      // window positions per SSIM workgroup
constexpr size_t kScoreWorkspaceBytes = 256u << 20;  // vfx_audio_metrics sub-batches its clips under this (vfx_handle::score_ws)
inline int sisdr_slabs(int64_t len) { return (int)((len + kSisdrSlab - 1) / kSisdrSlab); }
inline int ssim_tiles(int rows, int F) {  // the tiles of a (rows, F) image, rows and F >= 7
  return (rows - 6 + kSsimTileH - 1) / kSsimTileH * ((F - 6 + kSsimTileW - 1) / kSsimTileW);
}
struct ScoreFinalArgs {
  const int* lens = nullptr;              // samples per clip (the SI-SDR slabs)
  const int* frames = nullptr;            // rows per clip (the frame and SSIM sums)
  const double* sisdr_ws = nullptr;       // [B][nslab][3] or null (column 0 not written)
  int nslab = 0;
  const double* frames_ws[2] = {};        // [B][T][7] of the STFT rows, of the mel rows, or null (columns 1-3, 5-7)
  int T = 0;
  const double* ssim_ws[2] = {};          // [B][ssim_stride] tile sums of the two images, or null (columns 4, 8)
  int64_t ssim_stride[2] = {};
  int F[2] = {};
  double* out = nullptr;                  // [B][VFX_N_AUDIO_METRICS]
};
void launch_sisdr_slabs(const float* est, const float* tgt, int B, int64_t ld, const int* lens, int nslab, double* ws, hipStream_t s);
void launch_score_frames(const float* est, const float* tgt, int B, int T, int F, const int* frames, double* ws, hipStream_t s);
// ws [B][ssim_tiles(T, F)]
void launch_ssim_tiles(const float* est, const float* tgt, int B, int T, int F, const int* frames, double* ws, hipStream_t s);
void launch_score_final(const ScoreFinalArgs& a, int B, hipStream_t s);
// The four mel scores a handler writes per file (eval_gsr_voicefixer.py:59-64, eval_ssr_unet.py:116-126) for (B, T, 128) images, clip b =
// its first frames[b] rows (device, >= 7): out (B, VFX_N_HANDLER_METRICS) = mel-lsd, mel-sispec, mel-non-log-sispec, mel-ssim.
// ws: handler_metrics_ws_bytes(B, T) bytes, 256-byte aligned (the per-frame sums, then the SSIM tile sums).
//   launch_handler_metrics  the GSR handler's operand mix: lg = the model's log10 estimate, den = what the vocoder receives, tgt = the
//                           target's linear mel (k_handler_frames, k_ssim_tiles on (den, tgt), k_handler_final)
//   launch_mel_metrics      the SSR handler's: all four of (est, tgt) (k_score_frames, k_ssim_tiles, k_handler_final)
size_t handler_metrics_ws_bytes(int B, int T);
void launch_handler_metrics(const float* lg, const float* den, const float* tgt, int B, int T, const int* frames, char* ws, double* out,
                            hipStream_t s);
void launch_mel_metrics(const float* est, const float* tgt, int B, int T, const int* frames, char* ws, double* out, hipStream_t s);
int64_t count_nonfinite(const float* p, int64_t n, hipStream_t s);  // debug aid, synchronises

// losses.hip: the validation losses (vfx_spec_losses, vfx_validate_gsr_varlen).  Per-clip partial sums (float64) in ws; lens, n, counts,
// frames: device, [B]
constexpr int kL1Chunk = 4096;  // elements of a row per partial sum of k_l1_rows, cut from the row's own start
constexpr int kLossMaxClips = 128;  // clips per launch set of the two entries: what bounds their scratch (a clip's numbers do not depend on it)
inline int l1_chunks(int64_t n) { return (int)((n + kL1Chunk - 1) / kL1Chunk); }
// est, tgt (B, L), pair b = the first lens[b] samples -> ws (B, T, 2): per frame t < lens[b] / hop + 1 the sums over the 1025 bins of
// |se - st| and |log10 se - log10 st|, se / st = launch_stft_mel's magnitudes (eps) of the two clips, bit for bit; no spectrum is stored
void launch_pair_stft_l1(const FrontEndTables& t, const float* est, const float* tgt, int B, int L, int T, const int* lens, int hop,
                         float eps, double* ws, hipStream_t s);
// a, b (B, ld), row r = its first n[r] elements -> ws (B, nchunk): sum |float32(a_i - b_i)| per chunk of kL1Chunk elements
void launch_l1_rows(const float* a, const float* b, int B, int64_t ld, const int* n, int nchunk, double* ws, hipStream_t s);
// out[b * stride] = clip b's chunk sums / counts[b] (chunk_ws given); out[b * stride + col + {0, 1}] = its frame sums / (frames[b] * nbins)
// (frame_ws given)
void launch_loss_final(const double* chunk_ws, int nchunk, const int* counts, const double* frame_ws, int T, const int* frames, int nbins,
                       int col, double* out, int stride, int B, hipStream_t s);

// splice.hip: the level match of the splice (vfx_band_power).  a, b (B, L), pair p = the first lens[p] samples of both rows -> out (B, 2):
// the sums over its frames[p] = lens[p] / hop + 1 frames and the bins lo[p] <= k < hi[p] of |A|^2 and |B|^2 in float64, the magnitudes
// launch_stft_mel's (eps), bit for bit; lens, lo, hi, frames: device, [B]; ws: B * T * 2 doubles.  No spectrum is stored.
constexpr int kSpliceMaxClips = 128;  // clips per launch set of vfx_stft_splice and vfx_band_power (a clip's numbers do not depend on it)
void launch_pair_band_power(const FrontEndTables& t, const float* a, const float* b, int B, int L, int T, const int* lens, const int* lo,
                            const int* hi, const int* frames, int hop, float eps, double* ws, double* out, hipStream_t s);

// band.hip: the bandwidth detector (vfx_band_energy). The clips' lengths travel as kernel arguments, at most kBandMaxClips per launch
// set (clip_batch.h).
constexpr int kBandFrames = 8;      // consecutive frames of a clip per wave of k_band_energy: a constant, so that which frames a partial
                                    // sum holds depends on the clip alone
constexpr int kBandMaxClips = 128;  // clips per launch set
inline int band_groups(int len, int hop) { return (len / hop + 1 + kBandFrames - 1) / kBandFrames; }  // partial sums per bin of a clip
// wav (nb, ld), clip b = its first len[b] samples (len: HOST, nb <= kBandMaxClips, n_fft/2 < len[b] <= ld) -> energy (nb, 1025) or
// NULL, cut_bin (nb).  groups >= band_groups(len[b], hop) for every b; ws: nb * groups * 1025 doubles.
void launch_band_energy(const FrontEndTables& t, const float* wav, int nb, int64_t ld, const int* len, int hop, double threshold,
                        int groups, double* ws, double* energy, int* cut_bin, hipStream_t s);

// activity.hip: the peak-threshold silence functions (vfx_trim_bounds, vfx_long_empty, vfx_active_frames).  A mode names the window
// grid of a clip of n samples -- windows of W samples every S, the first at activity_origin, activity_windows of them:
//   ACT_TAIL, ACT_BOTH  the grid that ends at n: origin n % W, stride W (ACT_BOTH adds the grid from 0 behind it)
//   ACT_HEAD            the grid from 0, stride W; only whole windows
//   ACT_LONG            [L - W, L) for L = n, n - S, ... while L > W, in ascending order of position
//   ACT_FRAMES          the frames of the clip reflect-padded by S on both sides, from padded index 0 while a frame fits
enum { ACT_TAIL = 0, ACT_HEAD = 1, ACT_BOTH = 2, ACT_LONG = 3, ACT_FRAMES = 4 };  // the first three are VFX_TRIM_*
constexpr int kActMaxClips = 128;  // clips per launch set (clip_batch.h)
inline int64_t activity_windows(int mode, int64_t n, int64_t W, int64_t S) {
  if (mode == ACT_LONG) return n > W ? (n - W - 1) / S + 1 : 0;
  if (mode == ACT_FRAMES) return n + 2 * S >= W ? (n + 2 * S - W) / S + 1 : 0;
  return n / W;
}
inline int64_t activity_origin(int mode, int64_t n, int64_t W, int64_t S) {
  if (mode == ACT_LONG) return n > W ? n - W - (activity_windows(mode, n, W, S) - 1) * S : 0;
  if (mode == ACT_FRAMES) return -S;
  return mode == ACT_HEAD ? 0 : n % W;
}
// x (B, ldx) float32 or float64, clip b = its first lengths[b] samples (HOST; the caller has checked them with check_clip_lengths, and
// lengths[b] > S for ACT_FRAMES) -> the outputs of the mode: start, stop (B) for the trims (-1 / -1 = None), flag (B) for ACT_LONG,
// labels (B, ldf) and counts (B, or NULL) for ACT_FRAMES, everything device.  threshold: already rounded to x's dtype.  ws: (2 for
// ACT_BOTH, else 1) * min(B, kActMaxClips) * ldp elements of x's size, ldp >= activity_windows of every clip.
void launch_activity(int mode, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, int64_t W, int64_t S,
                     double threshold, void* ws, int64_t ldp, int64_t* start, int64_t* stop, int* flag, uint8_t* labels, int64_t ldf,
                     int64_t* counts, hipStream_t s);

// stft_dft.hip: the front end of the scores at 16 kHz (vfx_audio_metrics_rate): |STFT| with n_fft 743, hop 160 as a DFT-matrix GEMM on
// the f32-input MFMA, and the 80-band mel image.  An odd n_fft pads 371 samples on each side: 1 + (len - 1) / 160 frames.
constexpr int kDftN = 743, kDftHop = 160, kDftBins = kDftN / 2 + 1, kDftMels = 80, kDftRate = 16000;
constexpr int kDftK = 744;      // rows of the table: n, padded with a zero row to the MFMA's k step
constexpr int kDftCols = 384;   // columns per part (w cos | -w sin) of the table: the bins padded to 12 tiles of 32
constexpr int kDftStrip = 64;   // frames per workgroup
constexpr int kDftMinLen = 6 * kDftHop + 1;  // 7 frames (the smallest SSIM image), and more than the 371-sample reflection
__host__ __device__ inline int dft_frames(int len) { return 1 + (len - 1) / kDftHop; }
// Where entry (n, bin, part: 0 = w cos, 1 = -w sin) of the (kDftK, 2 kDftCols) table sits: in MFMA fragment order.  A pass of the K loop
// is 8 values of n = 4 k steps; the lane (bin, half) of a B fragment takes n = n0 + 2 k + half, k < 4, of both parts: 8 floats side by
// side, the lanes of a half wave 32 bytes apart.
constexpr int kDftPass = 8;
inline size_t dft_table_index(int n, int bin, int part) {
  const int pass = n / kDftPass, half = n & 1, k = (n % kDftPass) >> 1;
  return (((size_t)pass * 2 + half) * kDftCols + bin) * kDftPass + part * (kDftPass / 2) + k;
}
struct Score16kTables {
  float* table = nullptr;    // kDftK x 2 kDftCols floats at dft_table_index: the periodic Hann window times cos and -sin of
                             // 2 pi (k n mod 743) / 743; row 743 and the bins from 372 up are zeros
  float* fb_val = nullptr;   // packed non-zeros of the (372, 80) mel filterbank, band-major, as FrontEndTables'
  int* fb_start = nullptr;   // [80]
  int* fb_off = nullptr;     // [81]
  std::vector<float> fb_host;  // (372, 80) as loaded ("mel16k.fb" of VFX_MODEL_FRONTEND); empty: the float64 HTK table
};
// wav (B, L), clip b = its first lens[b] samples (kDftMinLen <= lens[b] <= L; lens: device) -> sp (B, T, 372), mel (B, T, 80); rows at
// or past a clip's dft_frames are zeros.  A frame's values depend on its clip's samples alone.
void launch_stft_dft(const Score16kTables& t, const float* wav, int B, int L, int T, const int* lens, float* sp, float* mel,
                     hipStream_t s);

// stoi.hip: STOI (Taal, Hendriks, Heusdens, Jensen 2011) of the clips of a padded batch, float64 from the first multiply on
constexpr int kStoiRate = 10000, kStoiFrame = 256, kStoiHop = 128, kStoiBands = 15, kStoiSegment = 30;
constexpr int kStoiMaxUp = 1024;        // reduced up factor: k_stoi_resample stages the phases of whole tap steps in LDS
constexpr int kStoiMaxDown = 1 << 15;   // reduced down factor
constexpr int kStoiMaxTaps = 1 << 20;   // taps of the resampling filter
__host__ __device__ inline int64_t stoi_out_len(int64_t n, int up, int down) { return (n * up + down - 1) / down; }   // len(resample_poly(x[:n]))
inline int stoi_frames(int64_t n) { return n > kStoiFrame ? (int)((n - kStoiFrame + kStoiHop - 1) / kStoiHop) : 0; }  // range(0, n - 256, 128)
// one intermediate of a vfx_stoi call, copied out for libvfx_test.so (vfx_op_stoi_stage; the stages and layouts: include/vfx_test.h)
struct StoiStageOut {
  int stage = 0;
  double* out = nullptr;
  int64_t out_n = 0;
  int* iout = nullptr;
  int64_t iout_n = 0;
};
// vfx_stoi (checks its arguments before the first launch); stage: null, or the intermediate to copy out (one sub-batch only)
void stoi_scores(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int up, int down,
                 const double* taps, int ntaps, double* out, const StoiStageOut* stage, hipStream_t s);

// bsseval.hip: BSS Eval v4 "images" SDR, ISR, SAR (Vincent, Gribonval, Fevotte 2006) of the clips of a padded batch, float64 throughout;
// the slabs of its sums are VFX_BSSEVAL_SLAB samples (include/vfx.h)
constexpr int kBssMaxFlen = 512;        // taps of the distortion filter: two MFMA accumulators of 256 lags per correlation
// one intermediate of a vfx_bsseval call, copied out for libvfx_test.so (vfx_op_bsseval_stage; the stages and layouts: include/vfx_test.h)
struct BssStageOut {
  int stage = 0;
  double* out = nullptr;
  int64_t out_n = 0;
};
// vfx_bsseval (checks its arguments before the first launch); stage: null, or the intermediate to copy out (one sub-batch only)
void bsseval_scores(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int flen, double* out,
                    const BssStageOut* stage, hipStream_t s);
void launch_chunk_gather(const float* x, int B, int L, int win, int hop, int lead, int n_chunks, float* chunks,
                         hipStream_t s);
void launch_chunk_ola(const float* frames, const float* window, float scale, int B, int n_chunks, int win, int hop,
                      int lead, int L, float* y, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// polyphase resampler (resample.hip): scipy.signal.resample_poly's arithmetic, bit for bit
// ---------------------------------------------------------------------------------------------
struct ResamplePair {
  int up, down;  // reduced by their gcd
  int hl;        // half filter length, 10 * max(up, down): the filter has 2 hl + 1 taps
  int R;         // outputs per lane of k_resample_poly; 0 = the filter does not fit the LDS budget (the pair is refused)
};
// false for up or down <= 0 (or beyond 2^20 after the reduction)
bool resample_reduce(int64_t up, int64_t down, ResamplePair* out);
int64_t resample_out_len(int64_t n_in, const ResamplePair& p);  // ceil(n_in up / down) = len(resample_poly(x[:n_in]))
// The one rule of the output-window form: the input indices [k0, k1) that outputs [o0, o0 + n) of a clip of n_in samples read
// (0 <= k0 <= k1 <= n_in; every index in it is read by one of those outputs; k0 = k1 = 0 when none is -- outputs past the clip's
// end are zeros)
void resample_window(int64_t n_in, const ResamplePair& p, int64_t o0, int64_t n, int64_t* k0, int64_t* k1);

constexpr int kResampleMaxClips = 64;  // clips per launch: their lengths are kernel arguments (the slices of clip_batch.h)
struct ResampleArgs {
  const float* x;     // (clips, ldx): global input indices [x0, x0 + Lx) of each clip
  const float* taps;  // 2 hl + 1
  float* y;           // (clips, ldy): global output indices [o0, o0 + n_out)
  int64_t ldx, x0, Lx, ldy, o0, n_out;
  int up, down, hl, span_max;
  int64_t lens_in[kResampleMaxClips], lens_out[kResampleMaxClips];
};
// x, y, taps: device; lens_in: HOST (B).  The caller has checked that [x0, x0 + Lx) holds what resample_window asks for.
void launch_resample(const float* x, int B, int64_t ldx, int64_t x0, int64_t Lx, const int64_t* lens_in, const ResamplePair& p,
                     const float* taps, float* y, int64_t ldy, int64_t o0, int64_t n_out, hipStream_t s);

// The per-clip form (k_resample_each): a rate pair per clip, float32 or float64, the taps in global memory.
constexpr int kResampleEachMaxClips = 128;     // clips per call: their parameters travel in a device table
constexpr int kResampleEachMaxDesigns = 128;
constexpr int kResampleEachMaxRate = 65536;    // max(up, down) after the gcd: what 44.1 / 48 kHz "stft" cut-offs need
constexpr int kResampleEachBlock = 256;        // outputs per workgroup, one per lane
struct ResampleEachDesign {  // one design of the call, for k_resample_each_taps
  int64_t src, dst;          // elements: the unscaled firwin in the caller's taps, the scaled copy in the handle's buffer
  int up, ntaps, J, pad_;    // J = 2 hl / up + 1: the row length of the phase-major copy
};
struct ResampleEachClip {    // one clip of the call, for k_resample_each
  int64_t x_at, y_at;        // elements: the clip's input and output row
  int64_t len_in, len_out;
  int64_t taps_at;           // elements: its design's scaled copy
  int up, down, hl, J;
  int64_t pad_;
};
// up / down reduced by their gcd, hl = 10 max(up, down); false for up or down <= 0 or max(up, down) > kResampleEachMaxRate after it
bool resample_each_reduce(int64_t up, int64_t down, ResamplePair* out);
// x, y (x's dtype), taps (x's dtype): device; lens_in, pair_index (B), pairs (F, reduced), taps_at (F): HOST.  The caller has checked
// 1 <= B <= kResampleEachMaxClips, 1 <= F <= kResampleEachMaxDesigns, the indices, 0 < n_out <= ldy and, with check_clip_lengths
// (api.cpp), 0 <= lens_in[b] <= ldx.
// y[b, n] for n < n_out: resample_poly's output n of clip b, zero at or past the clip's output length.
void launch_resample_each(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lens_in, const int* pair_index,
                          const ResamplePair* pairs, const void* taps, const int64_t* taps_at, int F, void* y, int64_t ldy, int64_t n_out,
                          hipStream_t s);

// ---------------------------------------------------------------------------------------------
// zero-phase IIR filter (sosfilt.hip): scipy.signal.sosfiltfilt's arithmetic, bit for bit
// ---------------------------------------------------------------------------------------------
constexpr int kSosTile = 64;          // samples per LDS tile of a clip (one wave-wide row)
constexpr int kSosMaxSections = 16;
constexpr int kSosMaxClips = 128;     // clips per launch: their lengths are kernel arguments
int sosfilt_clips_per_wave(int S);    // 4 rows of min(16 / S, 8) clips
// x (float32 or float64), f, y: device; lengths, sos (S, 6), zi (S, 2): HOST.  f (min(B, kSosMaxClips), ldf) receives the forward pass
// over the extended clips, ldf >= max length + 2 padlen.  The caller has checked 1 <= S <= 16 and, with check_clip_lengths (api.cpp),
// padlen < lengths[b] <= min(ldx, ldy).
// Both passes of every clip; y[b, lengths[b] .. ldy) = 0.
void launch_sosfiltfilt(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const double* sos, int S, const double* zi,
                        int padlen, double* f, int64_t ldf, double* y, int64_t ldy, hipStream_t s);
// The bank form: clip b takes design filter_index[b] of F designs, each with its own section count and padlen.
constexpr int kSosMaxDesigns = 128;
constexpr int kSosBankRow = 7;        // doubles per section of the device bank: b0 b1 b2 a1 a2 zi0 zi1
constexpr int kSosMaxBlocks = kSosMaxClips / 4 + kSosMaxSections;  // a block takes 4 clips of ONE section count: <= 48 per launch
// sos (F, Smax, 6), zi (F, Smax, 2) HOST -> bank (F, Smax, kSosBankRow) HOST, what the kernel reads from device memory
void sosfilt_pack_bank(const double* sos, const double* zi, int F, int Smax, double* bank);
// x, f, y, bank (sosfilt_pack_bank's, uploaded): device; lengths, filter_index (B), sections, padlens (F): HOST.  f as above with
// ldf >= max(length + 2 padlen of the clip's design).  The caller has checked the indices, 1 <= sections[.] <= Smax <= 16,
// lengths[b] <= min(ldx, ldy) with check_clip_lengths (api.cpp) and padlens[filter_index[b]] < lengths[b].  One launch pair per
// kSosMaxClips clips, whatever their section counts.
void launch_sosfiltfilt_bank(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* filter_index,
                             const double* bank, int Smax, const int* sections, const int* padlens, double* f, int64_t ldf, double* y,
                             int64_t ldy, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// room-impulse-response convolution (reverb.hip): direct form on the f32-input MFMA
// ---------------------------------------------------------------------------------------------
constexpr int kReverbTile = 8192;       // outputs per workgroup: 4 waves x 2 accumulators of 32 x 32
constexpr int kReverbTapBlock = 1024;   // taps per f32 fma chain; the block sums are combined in float64
constexpr int kReverbMaxTaps = 1 << 20; // longest RIR the entry point takes
constexpr int kReverbMaxClips = 128;    // clips per launch: their lengths are kernel arguments
// x, rirs, y, peaks: device; lengths (B), rir_lengths (R), rir_index (B, or NULL = b % R): HOST.  The caller has checked
// 1 <= lengths[b] <= min(ldx, ldy) with check_clip_lengths (api.cpp), 1 <= rir_lengths[r] <= min(ldr, kReverbMaxTaps) and the indices.
// Row b of y receives the first lengths[b] samples of clip b * rir, zeros up to ldy; peaks[b] (NULL: not wanted, normalize = 0 only)
// the largest |sample| of the whole convolution; normalize: rows whose peak exceeds 0.99 are scaled to a peak of 0.98.
void launch_reverb_rir(const float* x, int B, int64_t ldx, const int64_t* lengths, const float* rirs, int64_t ldr,
                       const int64_t* rir_lengths, const int* rir_index, int R, int normalize, float* y, int64_t ldy, float* peaks,
                       hipStream_t s);

// ---------------------------------------------------------------------------------------------
// noise mixing (mix.hip): add_noise_and_scale and its with_HQ / with_HQ_with_Aug forms
// ---------------------------------------------------------------------------------------------
constexpr int kMixMaxClips = 128;   // clips per launch: their lengths, weights and scales are kernel arguments
constexpr int kMixPeaks = 8;        // peak slots per clip: front, noise, hq, aug, the mixture (+ padding)
size_t mix_workspace_bytes(int B, int64_t lmax);  // of `ws` below, for B clips of at most lmax samples
// in (front, noise, hq, aug), out (front, noise, hq, aug, noisy): device (B, ld) or NULL; lengths, noise_weight (or NULL), scale: HOST (B).
// The caller has checked the form's pointers and, with check_clip_lengths (api.cpp), 1 <= lengths[b] <= ld.  Rows of every given output
// are zero from lengths[b] up to ld.
void launch_mix_noise(int form, int B, int64_t ld, const int64_t* lengths, const float* const in[4], const double* noise_weight,
                      const double* scale, float* const out[5], char* ws, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// array effects (effects.hip): MagicalEffects.quantification and time_dropout
// ---------------------------------------------------------------------------------------------
constexpr int kFxMaxClips = 128;   // clips per launch: their lengths, bins and indices are kernel arguments
constexpr int kFxMaxBins = 16;     // level = 2 ** bins <= 65536
constexpr int kFxSmoothHalf = 50, kFxSmoothStep = 4;                                       // smooth()'s smooth_samples and interval
constexpr int kFxSmoothKnots = 2 * kFxSmoothHalf / kFxSmoothStep;                          // 25 knots: patch[0], patch[4], .., patch[96]
constexpr int kFxSmoothRows = (kFxSmoothKnots - 1) * kFxSmoothStep;                        // 96 samples written: patch[0 .. 95]
// x, y, peaks (or NULL), bits (B slots): device; lengths, bins: HOST (B).  The caller has checked 1 <= lengths[b] <= min(ldx, ldy) with
// check_clip_lengths (api.cpp) and 0 <= bins[b] <= kFxMaxBins.  y[b, lengths[b] .. ldy) = 0.
void launch_quantize(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* bins, double* y, int64_t ldy,
                     void* peaks, unsigned long long* bits, hipStream_t s);
// x, y (x's dtype), smooth (kFxSmoothRows, kFxSmoothKnots): device; lengths, starts, ends: HOST (B).  The caller has checked the lengths
// with check_clip_lengths (api.cpp), as above, and 0 <= starts[b] <= ends[b].  y[b, lengths[b] .. ldy) = 0.
void launch_time_dropout(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int64_t* starts, const int64_t* ends,
                         const double* smooth, void* y, int64_t ldy, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// effect chain (chain.hip): the biquads, clip and reverse of MagicalEffects' sox chain, a program per clip
// ---------------------------------------------------------------------------------------------
constexpr int kChainMaxOps = 8;                    // steps of one clip's program
constexpr int kChainMaxStages = 4;                 // biquads of one launch of the cascade = of one sox run
constexpr int kChainMaxClips = 128;                // clips per set of launches: their passes are kernel arguments
constexpr int kChainMaxPasses = kChainMaxOps + 1;  // passes over one clip (a program of clips alone: the reduction, then one per clip)
enum ChainEnd : uint8_t { CHAIN_NONE = 0, CHAIN_BUF0 = 1, CHAIN_BUF1 = 2, CHAIN_CALLER = 3 };  // where a pass reads (x) or writes (y)
// One pass over one clip, in the order the kernels apply it: read at i, or at len - 1 - i (rev); clamp to the float32 bounds
// (min, max of what pass stat_in stored) * factor (clamp); widen and limit to sox's range (limit); nbq biquads, each output limited;
// round to float32 (round32; what goes to y always is); store, and leave the minimum and maximum of what was stored (stats).
struct ChainPass {
  double coef[kChainMaxStages][5];  // b0 b1 b2 a1 a2
  float factor;
  int row, slot, len;               // row of x and y; the clip's place in its slice: its row of the scratch and of the statistics
  int stat_in, stat_out;            // slot * kChainMaxPasses + the pass's number
  uint8_t nbq, rev, clamp, limit, round32, stats, src, dst;
};
// lengths, ops (B, K), coef (B, K, 5): HOST.  Cuts every program into passes: first[b] .. first[b + 1] of `passes` are clip b's.
// Throws for an unknown op and for more than kChainMaxStages biquads in one run.
void chain_plan(int B, const int64_t* lengths, const int* ops, const double* coef, int K, std::vector<ChainPass>& passes,
                std::vector<int>& first);
// x, y, tab (the uploaded passes), buf0, buf1 (min(B, kChainMaxClips), lds) doubles or NULL where no pass names them, stats
// (kChainMaxClips * kChainMaxPasses * 2): device.  The caller has checked 1 <= lengths[b] <= min(ldx, ldy) with check_clip_lengths
// (api.cpp).  Per slice of kChainMaxClips clips: round r runs pass r of every clip that has one, the cascades in one grid, the
// element-wise passes in another.  y[b, lengths[b] .. ldy) = 0.
void launch_effect_chain(const float* x, int64_t ldx, int B, const std::vector<ChainPass>& passes, const std::vector<int>& first,
                         const ChainPass* tab, double* buf0, double* buf1, int64_t lds, unsigned* stats, float* y, int64_t ldy,
                         hipStream_t s);

// ---------------------------------------------------------------------------------------------
// handle-side data structures
// ---------------------------------------------------------------------------------------------
struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// Long-lived device allocations (tables, weights, plan parameter blocks).
struct DeviceBlob {
  std::vector<void*> allocs;
  void* alloc(size_t bytes);
  float* upload(const float* p, size_t n);
  float* upload(const std::vector<float>& v) { return upload(v.data(), v.size()); }
  int* upload_i(const std::vector<int>& v);
  void release();
  ~DeviceBlob() { release(); }
};

// Offsets into the workspace arena, assigned at plan-build time by a first-fit free list.
struct ArenaPlanner {
  struct Block { size_t off, size; bool free; };
  std::vector<Block> blocks;
  size_t high = 0;
  size_t alloc(size_t bytes);
  void free(size_t off);
};

// A device buffer of the handle that only grows.  Growing synchronises, frees and re-allocates, so nothing may keep a pointer into
// it across a call that may grow it -- except the plans a hipGraph was captured from, which is why a buffer they point into refuses.
struct GrowBuffer {
  char* p = nullptr;
  size_t bytes = 0;
  // -> the buffer, at least `need` bytes; a buffer that has to grow takes need + need / slack_div bytes (0: no slack).  pinned_msg
  // (format: old size, new size, plan key) or NULL: the error when it has to grow while a plan of `h` is pinned.  h->arena alone also
  // drops the retired plans and takes the poison fill of VFX_TUNE_DEBUG_POISON_ARENA.
  char* ensure(vfx_handle* h, size_t need, size_t slack_div, const char* pinned_msg = nullptr);
  GrowBuffer() = default;
  ~GrowBuffer() {
    if (p) (void)hipFree(p);
  }
  GrowBuffer(const GrowBuffer&) = delete;
  GrowBuffer& operator=(const GrowBuffer&) = delete;
};

// A table of a call that is too large for a kernel-argument block: a device buffer of the handle that only grows, filled on the
// call's stream from pinned host memory of the handle.  stage() hands out the pinned memory -- after waiting, on the host, for the
// previous upload's copy to have read it --, upload() enqueues the copy and returns the device table for the launches that follow
// on that stream.  (Calls on other streams take turns behind it: StreamTurn.)
struct StagedUpload {
  GrowBuffer dev;
  char* host = nullptr;
  size_t host_bytes = 0;
  hipEvent_t copied = nullptr;
  bool pending = false;
  char* stage(vfx_handle* h, size_t bytes);
  char* upload(size_t bytes, hipStream_t s);
  StagedUpload() = default;
  ~StagedUpload() {
    if (host) (void)hipHostFree(host);
    if (copied) (void)hipEventDestroy(copied);
  }
  StagedUpload(const StagedUpload&) = delete;
  StagedUpload& operator=(const StagedUpload&) = delete;
};

// One launch of a profiled call (vfx_profile_*): HIP events around it, its work, and its row of the VFX_PROFILE_DUMP table.
struct LaunchRecord {
  hipEvent_t begin, end;
  double flops;
  double bytes;         // algorithmic HBM bytes of the launch
  double design_bytes;  // what the kernel's data layout moves (two-form trunks carry their fp16 copies)
  char kernel[64];
  int M, Cout, K, nseg, ntaps0, C0, Wi, sw;
};
struct ConvProfile {  // HIP-event timing of every convolution launch
  bool enabled = false;
  std::vector<LaunchRecord> launches;
};

// A buffer is either a slice of the arena (resolved when the plan is bound to an arena base)
// or one of the caller's tensors (resolved per call).

struct RunCtx {
  hipStream_t stream;
  float* ext[8];
  int* flags;
  ConvProfile* prof = nullptr;
};

struct Plan {
  std::vector<std::function<void(const RunCtx&)>> ops;
  std::vector<TapConvParams> host_params;  // arena-relative until bind()
  std::vector<TapConvParams> abs_params;   // the same with absolute pointers, as uploaded by bind()
  TapConvParams* dev_params = nullptr;
  ConvStage* dev_stages = nullptr;
  std::map<size_t, std::vector<TapSeg>> phase_segs;  // phased launches: host_params index -> per-phase segment
  std::vector<ResBlockParams> host_rb;     // arena-relative until bind()
  ResBlockParams* dev_rb = nullptr;
  DeviceBlob blob;
  size_t arena_bytes = 0;
  char* bound_base = nullptr;
  double conv_flops = 0;
  int n_conv = 0;
  std::map<std::string, size_t> named;  // named arena offsets (bytes) of stage-level buffers
  uint64_t last_use = 0;                // handle tick of the last call (LRU eviction, get_plan)
  bool pinned = false;                  // a hipGraph was captured from this plan: its parameter blocks must outlive the graph
  void run(const RunCtx& ctx);  // plan.cpp (debug hooks: VFX_POISON_ARENA=2, VFX_DEBUG_NAN)
};

// Arena-relative pointer encoding used inside TapConvParams until bind_plan(): offset + 1
// (so that offset 0 is distinguishable from nullptr).
inline const float* rel_ptr(size_t off) { return reinterpret_cast<const float*>(off + 1); }

// A tap convolution as a builder function hands it to the plan: phases empty = PlanBuilder::add_conv, otherwise add_conv_phased
struct ConvLaunch {
  TapConvParams p;
  std::vector<TapSeg> phases;
};

struct PlanBuilder {
  vfx_handle* h;
  Plan* plan;
  ArenaPlanner arena;
  int short_clip = 0;  // copied into every TapConvParams added from here on (TapConvParams::short_clip)
  // Batches of clips of unequal length (vfx_restore_gsr_varlen): device arrays [B] of the handle, refilled by every call --
  // frames per clip (T_b = L_b / hop + 1) and vocoder frames per clip (T_b + T_b % 2 + 4).  NULL: every clip has the plan's T.
  const int* lens_t = nullptr;
  const int* lens_tp = nullptr;
  // set by build_vocoder: its launches never split K (split-K is the deep ResUNet levels' tool; a vocoder launch of a short clip
  // would otherwise sum in another order than the same clip inside a varlen batch, whose launches cannot split -- with this
  // every arithmetic mode gives a clip the same bits in both entry points)
  bool no_splitk = false;
  // returns arena offset in BYTES
  size_t alloc_f(int64_t nfloat) { return arena.alloc((size_t)nfloat * sizeof(float)); }
  void free(size_t off) { arena.free(off); }
  // Adds a tap-convolution whose src/residual/out pointers are arena offsets encoded as
  // (const float*)offset; they are rebased in Plan::bind.
  void add_conv(TapConvParams p);
  // p.seg[0] carries the UNION of the phases' taps (geometry only); phases[r] = source / prologue / taps / weights of phase r
  void add_conv_phased(TapConvParams p, const std::vector<TapSeg>& phases);
  void add_conv(const ConvLaunch& l) { l.phases.empty() ? add_conv(l.p) : add_conv_phased(l.p, l.phases); }
  void add_resblock(ResBlockParams p);  // x / y are arena offsets encoded with rel_ptr()
};

struct ConvBlockW {
  int cin = 0, cout = 0, nsrc = 1;  // nsrc = 2: the input is cat(src0, src1), cin/2 channels each
  float *bn1_scale = nullptr, *bn1_shift = nullptr, *bn2_scale = nullptr, *bn2_shift = nullptr;
  float* w1[2] = {nullptr, nullptr};   // conv1 packed per source
  float* w2 = nullptr;                 // conv2 packed
  float* wsc[2] = {nullptr, nullptr};  // 1x1 shortcut packed per source (cin != cout)
  float* bsc = nullptr;
  bool shortcut = false;
};

struct DecoderW {
  int cin = 0, cout = 0;
  float *bn_scale = nullptr, *bn_shift = nullptr;
  float* wT[4] = {nullptr, nullptr, nullptr, nullptr};  // packed per output parity class (a*2+b)
  ConvBlockW blocks[4];
};

struct UNetWeights {
  float c1_scale = 1.f, c1_shift = 0.f;
  float *c1_w = nullptr, *c1_wsc = nullptr, *c1_bsc = nullptr;
  ConvBlockW enc[6][4];
  ConvBlockW bott;
  DecoderW dec[6];
  ConvBlockW after;
  float* final_w = nullptr;
  float final_b = 0.f;
};

struct VocConvW {
  float* w = nullptr;     // packed (per phase for transposed convs: w_phase[r])
  float* bias = nullptr;  // [cout]; transposed convs: repeated once per output phase ([stride][cout])
  std::vector<float*> w_phase;
  int cin = 0, cout = 0;
  int mode = 0;  // pack_conv mode the weights were packed with (follows the form of the source tensor in the plan)
};

// Linear layers and GRUs of the bi_gru / dnn analysis modules (analysis.hip)
struct DenseW {
  int K = 0, N = 0;
  float* wT = nullptr;    // (K, N): the weight transposed
  float* bias = nullptr;  // (N)
};
struct AnalysisWeights {
  int model = 0;
  std::vector<DenseW> dense;  // bi_gru: Linear 1, GRU projections of layers 1 / 2 (N = 1536), Linear 4, 6; dnn: Linear 0, 3, .., 12, 14
  float bn_scale[4] = {1.f, 1.f, 1.f, 1.f}, bn_shift[4] = {0.f, 0.f, 0.f, 0.f};  // the BatchNorm2d(1) scalars in module order
  float* whhT[2] = {nullptr, nullptr};  // per GRU layer: (2 directions, 256, 768) W_hh transposed
  float* bhn[2] = {nullptr, nullptr};   // per GRU layer: (2, 256) b_hn
};

struct VocoderWeights {
  std::vector<VocConvW> cond;   // k3 convs
  VocConvW pre;                 // k7 reflect
  std::vector<VocConvW> up;     // transposed convs
  std::vector<std::vector<std::pair<VocConvW, VocConvW>>> res;
  float* final_w = nullptr;     // [7][C]
  float final_b = 0.f;
  int final_c = 0;
  bool needs_strict = false;    // 16-bit mode: a weight tensor does not fit fp16 operands (f16_weight_issue)
};

// The vocoder's launches (vocoder.cpp), built by the plan (build_vocoder) and by the parity entry points of libvfx_test.so from the
// same functions: buffer pointers are the caller's (arena-relative rel_ptr() offsets in a plan, device pointers in a test).
// Taps (e, k) of output phase r of ConvTranspose1d(k = 2s, stride s, padding pad): out[s q + r] += x[q - e] W[:, :, k]
std::vector<std::pair<int, int>> voc_phase_taps(int s, int pad, int r);
// PyTorch-layout weights (Conv1d (cout, cin, K); ConvTranspose1d (cin, cin / 2, 2 s)) and biases on the host -> packed for a source
// in activated form (src_act) or raw
VocConvW pack_voc_conv1d(const vfx_config& cfg, DeviceBlob& blob, const float* w, const float* bias, int cin, int cout, int K, bool src_act);
VocConvW pack_voc_upsampler(const vfx_config& cfg, DeviceBlob& blob, const float* w, const float* bias, int cin, int s, bool src_act);
// Conv1d (K, dilation dil, 'same' zero padding or reflect) on (B, T, cin): src activated (no prologue) or raw with prologue `act`
// (slope); residual raw, or -- residual_act -- the activated fp16 form LeakyReLU(res_slope) of the residual, inverted in the epilogue;
// raw output `out` and / or activated output `out_act` (next_act, next_slope); lens: per-clip lengths in units of `rate` positions.
TapConvParams voc_conv1d_params(const vfx_config& cfg, const VocConvW& cw, int B, int T, int K, int dil, bool reflect, const float* src,
                                bool src_act, int act, float slope, const float* residual, bool residual_act, float* out, float* out_act,
                                int next_act, float next_slope, const int* lens, int rate);
// ConvTranspose1d(k = 2s, stride s) on (B, T, cin) as ONE phased launch (PlanBuilder::add_conv_phased): returns p with seg[0] = the
// union window of the phases' taps, phases[r] = phase r.  Output (B, T, s * cout): raw `out` and / or activated `out_act` (act_slope;
// 1 = the fp16 trunk of the 16-bit mode); lens in INPUT positions per unit of `rate`.
TapConvParams voc_upsample_params(const vfx_config& cfg, const VocConvW& up, int s, int B, int T, const float* src, bool src_act,
                                  float* out, float* out_act, float act_slope, const int* lens, int rate, std::vector<TapSeg>& phases);
// 1 when the plan runs the upsampler of a cin-channel stage (behind the first, not the last) on k_up16, 0 on the phased k_conv
int voc_plan_upsampler_kernel(const vfx_config& cfg, int cin, int s, int T);
// One ResStack layer (conv1, conv2) of `channels` channels.  How the plan runs it: two k_conv launches, one fused launch on the raw
// trunk (resblock.hip, resblock_rw.hip, resblock_r128.hip) or one on the activated fp16 trunk (resblock_w64.hip); whether the tensors
// between the launches of its stack are fp16 (ResBlockParams::x16; last_stage: the stack feeds the vocoder tail); whether the layers
// of dilation dil, dil2 run as one launch.
using VocResLayer = std::pair<VocConvW, VocConvW>;
enum { VOC_RES_TWO_LAUNCHES = 0, VOC_RES_FUSED = 1, VOC_RES_FUSED_WIDE = 2 };
int voc_resblock_kind(const vfx_config& cfg, int channels);
bool voc_resblock_trunk_f16(const vfx_config& cfg, int channels, bool last_stage);
bool voc_resblock_pair_ok(const vfx_config& cfg, int channels, int dil, int dil2);
// The fused launch of layer l1 (dilation dil) -- and, l2 != NULL, of the layer behind it (dil2) in the same launch -- on (B, T, channels):
// the trunk form, slopes, operand mode and the pair fields.  x / y: the raw trunk in and out (fp32, or fp16 where
// voc_resblock_trunk_f16); xa / ya: the activated fp16 forms (xa: the wide layer's source; ya = fp16(LeakyReLU(y, act_slope)) for the
// next consumer).  A pointer is NULL where the plan keeps no such tensor: y of the last layer in front of an upsampler on the fp16
// trunk, x and y of the wide layer on it.  lens: per-clip lengths in units of `rate` positions.  plan_resblock() picks the kernel.
ResBlockParams voc_resblock_params(const vfx_config& cfg, int channels, bool last_stage, const VocResLayer& l1, const VocResLayer* l2, int B,
                                   int T, int dil, int dil2, const float* x, const float* xa, float* y, float* ya, float act_slope,
                                   const int* lens, int rate);
// The phased launch hp (after finish_params, with tuning set) with the phase segments `phases` runs on k_up16: upsample16_ok, two
// taps per phase and not VFX_TUNE_NO_FUSED_UPSAMPLERS (upsample16.hip)
bool upsample16_selected(const TapConvParams& hp, const std::vector<TapSeg>& phases);

// Conv weights -> MFMA fragment order [C/chunk][ntaps][Cout/32][1024 floats] (conv.hip); mode: 0 fp32, 1 split-bf16
// (hi | lo), 2 fp16 in the hi fragments (32-channel chunks, raw sources of the 16-bit mode), 3 fp16 with 64-channel
// chunks (activated fp16 sources of the 16-bit mode); conv_chunk(mode) = input channels per chunk.
int conv_chunk(int mode);
int stage_channels(const TapConvParams& p, const TapSeg& S);
std::vector<float> pack_conv(const float* w, int Cout, int CinTotal, int KH, int KW, int c_lo, int C,
                             const std::vector<std::pair<int, int>>& taps, int mode);
std::vector<float> pack_conv_transposed(const float* w, int Cin, int Cout, int KH, int KW,
                                        const std::vector<std::pair<int, int>>& taps, int mode);
void rows_to_fragments(std::vector<float>& packed, int Cout, int mode);  // [..][Cout][32] rows -> fragment order
// Set by rows_to_fragments when a tensor packed as fp16 operands (modes 2, 3) does not fit fp16 (|w| > 65504, or the whole
// tensor deep in the subnormal range); the weight builders reset it before and read it after packing a model.
bool& f16_weight_issue();
void launch_or_flags(int* flags, int bits, hipStream_t s);  // small_ops.hip: flags |= bits, in stream order

}  // namespace vfx

struct vfx_handle {
  int device = 0;
  vfx_config cfg{};
  std::map<std::string, vfx::HostTensor> staged[6];
  vfx::FrontEndTables fe;
  vfx::Score16kTables fe16;  // the 743-point front end of the scores at 16 kHz, built on first use (ensure_score16k_tables)
  vfx::DeviceBlob blob;  // front-end tables + weights
  std::shared_ptr<vfx::UNetWeights> unet[2];
  std::shared_ptr<vfx::VocoderWeights> voc;
  std::shared_ptr<vfx::AnalysisWeights> analysis[2];  // VFX_MODEL_GRU_MEL, VFX_MODEL_DNN_MEL
  int analysis_model = VFX_MODEL_UNET_MEL;             // what vfx_restore_gsr(_varlen) runs (vfx_select_analysis)
  std::map<std::string, std::shared_ptr<vfx::Plan>> plans;  // at most kMaxCachedPlans, least recently used evicted
  std::vector<std::shared_ptr<vfx::Plan>> retired;  // evicted plans whose device blocks are freed in batches (get_plan)
  uint64_t plan_tick = 0;
  vfx::GrowBuffer arena;     // the workspace the plans place their buffers in (bind_plan)
  int* d_flags = nullptr;
  int* d_lens = nullptr;     // [kLensRows][kMaxVarlenClips]
  int* lens_row(vfx::LensRow r) const { return d_lens + r * vfx::kMaxVarlenClips; }
  vfx::GrowBuffer scratch;   // the tensors between the plans of a varlen call (vfx_restore_gsr_varlen)
  vfx::GrowBuffer score_ws;  // vfx_audio_metrics' spectra and partial sums (<= kScoreWorkspaceBytes unless one clip needs more)
  vfx::GrowBuffer sos_ws;    // vfx_sosfiltfilt's forward pass over the extended clips (float64)
  vfx::StagedUpload sos_bank;  // vfx_sosfiltfilt_bank's designs: coefficients and zi of every section (sosfilt_pack_bank)
  vfx::GrowBuffer mix_ws;   // vfx_mix_noise's per-clip peaks, level ratios and chunk sums
  vfx::GrowBuffer fx_ws;    // vfx_quantize's per-clip peaks (bit patterns)
  vfx::StagedUpload fx_smooth;          // vfx_time_dropout's smoothing matrix on the device ...
  std::vector<double> fx_smooth_seen;   // ... and what it holds: uploaded again only when the caller's matrix differs
  vfx::GrowBuffer chain_ws;      // vfx_effect_chain's intermediate clips between passes (float64) and their minima and maxima
  vfx::StagedUpload chain_tab;   // vfx_effect_chain's passes (ChainPass)
  vfx::GrowBuffer rs_taps;  // vfx_resample_each's scaled taps of the designs of a call (at most 11 MB per design)
  vfx::StagedUpload rs_table;  // vfx_resample_each's design and clip tables
  bool rs_natural_taps = false;  // debug switch (vfx_debug_resample_each_layout): the scaled taps in natural order, not phase-major
  float* d_ones = nullptr;   // identity prologue tables (kIdentityLen floats)
  float* d_zeros = nullptr;
  vfx::ConvProfile prof;
};

namespace vfx {
void init_front_end(vfx_handle* h);
void set_mel_filterbank(vfx_handle* h, const float* fb /*1025x128*/);
// the tables of stft_dft.hip, uploaded on the first call; fb (372 x 80) or NULL: the filterbank to use from now on
const Score16kTables& ensure_score16k_tables(vfx_handle* h);
void set_score16k_filterbank(vfx_handle* h, const float* fb);
void bind_plan(vfx_handle* h, Plan& plan);  // ensures the arena is large enough and rebases the plan on it
std::string key_of(const char* tag, int B, int T, int x = 0);  // key of a cached plan (vfx_handle::plans)
// What a model-stage entry point does with a plan: take it from the handle's cache (building and binding it as needed: `build`),
// poison its arena bytes on a VFX_TUNE_DEBUG_POISON_ARENA handle, then -- behind `before`, if given: launches of the call that write
// the plan's named buffers -- run it on `stream` with the caller's tensors `ext` (RunCtx::ext).  Returns the plan (Plan::named).
std::shared_ptr<Plan> run_plan(vfx_handle* h, const std::string& key, void* stream, std::initializer_list<const float*> ext,
                               const std::function<void(PlanBuilder&)>& build, const std::function<void(Plan&)>& before = nullptr);
std::shared_ptr<UNetWeights> build_unet_weights(vfx_handle* h, int model);
std::shared_ptr<VocoderWeights> build_vocoder_weights(vfx_handle* h);
std::shared_ptr<AnalysisWeights> build_analysis_weights(vfx_handle* h, int model);

// plan builders: append the ops of one stage to `pb`.  Buffers named *_off are arena byte
// offsets; ext slots index RunCtx::ext.
//   unet: input = ext[in_slot] or arena (in_off); mel model writes (B,T,128) log-mel to ext[out_slot] / arena.
struct BufRef {
  bool ext = false;
  int slot = 0;
  size_t off = 0;
};
void build_unet_mel(PlanBuilder& pb, int B, int T, BufRef mel_linear, BufRef logmel_out);
void build_unet_spec(PlanBuilder& pb, int B, int T, BufRef sp, BufRef cosb, BufRef sinb, BufRef re_out, BufRef im_out);
// One piece of a ResUNet plan on its own, for libvfx_test.so (vfx_op_unet_piece, vfx_plan_unet_piece): appended by the member
// functions of the plan builder that build_unet_mel / build_unet_spec run (resunet.cpp), over input and output buffers of the
// piece's own in the arena, with pb's short_clip and lens_t.  name: "entry" (encoder_block1.conv_block1 on a (B, H, W) plane);
// "enc<l>.<j>", "bott", "after", "dec<d>.<j>" (j = 1: the two-source block behind the upsampler) = one ConvBlockRes on (B, H, W, Cin)
// sources; "dec<d>.up" = the upsampler (arg = prune_w) -> (B, 2H, 2W [+ 1], Cout); "pool" (arg = C); "prep_logmel" / "prep_spec"
// (H = T frames: (B, T, 128 / 1025) -> (B, Tpad, 127 / 1024)); "final" (H = T, W = the trunk's width, arg = mode: inputs the trunk's
// (B, Tpad, W, 32) output and the one (mode 0) or two (B, T, W + 1) planes of the epilogue -> one or two (B, T, W + 1) planes).
struct UNetPiece {
  const char* name;
  int B, H, W, arg;
  // filled by build_unet_piece: arena byte offsets and float counts of the buffers
  int nin, nout;
  size_t in_off[3], out_off[2];
  int64_t in_n[3], out_n[2];
  // the tensor between the two launches of a block's two-launch form (h_n = 0: there is none).  h_form 1: the ACTIVATED operand form
  // conv1 stores for conv2 (TapConvParams::out_act); 0: raw fp32 (the entry block's k_conv_c1)
  size_t h_off;
  int64_t h_n;
  int h_form;
};
void build_unet_piece(PlanBuilder& pb, const UNetWeights& Wt, UNetPiece& piece);
// The launches of a ResUNet upsampler (resunet.cpp: the one-launch, two-launch and four-launch forms), for the plans (no bias, BN + ReLU
// prologue) and for vfx_op_conv_transpose: prologue scale / shift [Cin] (NULL: identity) + act (slope) on src (B, H, W, Cin), weights
// wT[2 a + b] packed per output parity class, bias [Cout] or NULL -> out (B, 2H, prune_w ? 2W : 2W + 1, Cout).  src / out as the plan
// wants them (rel_ptr offsets); every launch goes to PlanBuilder::add_conv.
std::vector<ConvLaunch> unet_upsample_launches(int tuning, int B, int H, int W, int Cin, int Cout, bool prune_w, const float* src, float* out,
                                               const float* scale, const float* shift, int act, float slope, const float* const wT[4],
                                               const float* bias);
UNetWeights unet_weight_shapes();  // the channel counts of every block, no tensors: what build_unet_weights fills (host-only planning)
// What a piece's plan launches, in order: kUNetLaunchInts ints per launch = family (UNetLaunchFamily), ksplit (1 = none), activated
// output, bias, K segments, output channels.  Returns the number of launches; writes those that fit `cap` ints.
enum UNetLaunchFamily {
  UNET_LAUNCH_SMALL = 0, UNET_LAUNCH_CONV = 1, UNET_LAUNCH_CONV_PHASED = 2, UNET_LAUNCH_BLOCK = 3, UNET_LAUNCH_BLOCK_IN1 = 4,
  UNET_LAUNCH_BLOCK_TWO_SRC = 5, UNET_LAUNCH_BLOCK2D32 = 6
};
constexpr int kUNetLaunchInts = 6;
int describe_unet_launches(const Plan& plan, int* out, int cap);
void build_vocoder(PlanBuilder& pb, int B, int T, BufRef mel_linear, BufRef wav_out, const BufRef* peak = nullptr);
// bi_gru / dnn Generator.forward: linear mel (B,T,128) -> log-mel (B,T,128); pb.lens_t (frames per clip) or all T
void build_analysis_mel(PlanBuilder& pb, int model, int B, int T, BufRef mel_linear, BufRef logmel_out);
// The launches of those plans, one member each (analysis.hip): build_analysis_mel calls them in order, build_analysis_piece one of them.
// Tensors are (B, T, C) rows, fp32; every member appends one launch over pb.lens_t (frames per clip) or all T.
struct AnalysisBuilder {
  PlanBuilder& pb;
  const AnalysisWeights& W;
  int B, T;
  // bi_gru
  void lin1(BufRef mel, BufRef out);              // to_log + BN 0 -> Linear 1 -> BN 2.bn: (., 128) linear mel -> (., 256)
  void proj(int layer, BufRef src, BufRef xp);    // both directions' W_ih x + b_ih (+ b_hr, b_hz): (., 256 | 512) -> (., 1536)
  void gru(int layer, BufRef xp, BufRef out);     // k_gru_seq: (., 1536) -> (., 512) = [forward | backward]
  void lin4(BufRef src, BufRef out);              // ReLU -> Linear 4 -> ReLU: (., 512) -> (., 256)
  void lin6(BufRef src, BufRef mel, BufRef out);  // Linear 6, + to_log(mel): (., 256) -> (., 128)
  // dnn: layer i of 0..5 (Linear 3 i, or 14), widths 128, 256, 512, 1024, 512, 256, 128.  0: to_log in front; 0..4: ReLU behind, 0..3:
  // then the BN; 5: + to_log(mel) (mel is read by layer 5 alone)
  void fc(int i, BufRef src, BufRef mel, BufRef out);
  // one k_dense launch; resid: y += to_log(mel)
  void dense(const DenseW& d, BufRef src, BufRef dst, int in_log, float in_scale, float in_shift, int in_relu, int out_relu,
             float out_scale, float out_shift, bool resid, BufRef mel);
};
// One launch of an analysis plan on its own, for libvfx_test.so (vfx_op_analysis_piece): appended by the AnalysisBuilder member that
// build_analysis_mel runs, over input and output buffers of the piece's own in the arena, with pb's lens_t.  name: "lin1", "proj0",
// "gru0", "proj1", "gru1", "lin4", "lin6" (VFX_MODEL_GRU_MEL), "fc0" .. "fc5" (VFX_MODEL_DNN_MEL); "lin6" and "fc5" have two inputs,
// the second the linear mel.
struct AnalysisPiece {
  const char* name;
  int B, T;
  // filled by build_analysis_piece: arena byte offsets and float counts of the buffers
  int nin;
  size_t in_off[2], out_off;
  int64_t in_n[2], out_n;
};
void build_analysis_piece(PlanBuilder& pb, int model, AnalysisPiece& piece);
// d[0 .. B) = host[0 .. B) in stream order (kernel arguments: legal inside a stream capture); one row, unlike launch_set_lens
void launch_set_frames(int* d, const int* host, int B, hipStream_t s);
int64_t vocoder_out_len(const vfx_config& cfg, int T);
}  // namespace vfx
