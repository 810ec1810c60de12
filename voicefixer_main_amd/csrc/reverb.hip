// reverb.hip -- batched direct-form convolution of float32 clips with float32 room impulse responses on the f32-input MFMA (gfx950):
// the device form of MagicalEffects.reverb_rir (dataloaders/augmentation/magical_effects.py:158-167).
//
// Convolution as a GEMM whose operands are generated from the two 1-D arrays.  For 1024 consecutive outputs starting at t0 write
// n = t0 + 32 p + q and m = q + s:
//
//   y[t0 + 32 p + q] = sum over s of A[p][s] B[s][q],   A[p][s] = x[t0 + 32 p - s],   B[s][q] = h[q + s],   s in [-31, M - 1]
//
// A is zero outside [0, N), B outside [0, M): exact zeros, so the padding adds no error.  One 32 x 32 accumulator of
// v_mfma_f32_32x32x2_f32 holds the 1024 outputs; a k step of the instruction is two consecutive values of s.
//
// Accumulation rule: s runs in blocks of kReverbTapBlock values.  Within a block the accumulator starts from zero and the MFMA's own
// k-ordered f32 fma chain does the sum (at most min(M, kReverbTapBlock) non-zero terms per output: a block covers kReverbTapBlock
// consecutive taps of every output); the block sums are added in float64 in ascending block order and rounded to float32 once.  So
//   |y - truth| <= (min(M, kReverbTapBlock) + 2) 2^-24 sum |x||h| + 2^-149
// for any data, and a clip's result depends on the clip and its RIR alone, never on the batch.  A block whose x window lies wholly
// outside [0, N) is skipped: its sum is an exact zero.
//
// Work split: a workgroup of four waves computes kReverbTile = 8192 consecutive outputs of one clip, two accumulators per wave that
// share the B fragment.  Per tap block it stages the x window (kReverbTile + kReverbTapBlock - 32 samples) and the h block
// (kReverbTapBlock + 31 taps) in LDS.  The x window is kept in rows of 32 samples padded to 33 floats: lane p of an A fragment reads
// at a stride of 32 samples, which the pad turns into 33 banks apart.  The window's origin is chosen so that the 32 values of s of one
// pass of the inner loop stay inside one row for every lane: all 16 reads of a pass are one base address plus a constant.
//
// All N + M - 1 outputs of a clip are computed; the first N go to y, and every one of them -- rounded to float32 -- feeds the clip's
// peak through an atomicMax on the bit pattern of |y| (order-independent; a NaN lands above every finite value).  k_reverb_scale then
// does the reference's normalisation, (y / peak) * 0.98f where (double)peak > 0.99: NumPy's arithmetic on a float32 array.
#include "clip_batch.h"
#include "vfx_internal.h"

namespace vfx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kReverbWaves = 4, kReverbAcc = 2;  // accumulators (1024 outputs each) per wave
static_assert(kReverbTile == kReverbWaves * kReverbAcc * 1024, "a tile is the workgroup's accumulators");
static_assert(kReverbTapBlock % 32 == 0 && kReverbTapBlock <= 1024, "a pass of the inner loop is 32 values of s");
constexpr int kReverbXRows = kReverbTile / 32 + kReverbTapBlock / 32 - 1;  // rows of 32 samples of the x window
constexpr int kReverbXRow = 33;                                            // floats per LDS row
constexpr int kReverbHs = kReverbTapBlock + 32;

struct ReverbArgs {
  const float* x;     // (clips, ldx)
  const float* rirs;  // (R, ldr)
  float* y;           // (clips, ldy)
  unsigned* peaks;    // (clips) bit patterns of max |y32| over the full convolution, zeroed before the launch; or NULL
  int64_t ldx, ldr, ldy;
  int len[kReverbMaxClips], rir[kReverbMaxClips], rir_len[kReverbMaxClips];
};

__global__ __launch_bounds__(kReverbWaves * 64) void k_reverb(const ReverbArgs a) {
  __shared__ float smem[kReverbXRows * kReverbXRow + kReverbHs];
  float* const xs = smem;
  float* const hs = smem + kReverbXRows * kReverbXRow;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane & 31, half = lane >> 5;
  const int b = blockIdx.y;
  const int N = a.len[b], M = a.rir_len[b];
  const float* const x = a.x + (int64_t)b * a.ldx;
  const float* const h = a.rirs + (int64_t)a.rir[b] * a.ldr;
  float* const y = a.y + (int64_t)b * a.ldy;
  const int64_t t0l = (int64_t)blockIdx.x * kReverbTile;
  const int64_t nfull = (int64_t)N + M - 1;

  {  // zeros from the clip's length up to ldy: this tile's share, the last tile of the grid takes what lies beyond the grid
    const int64_t lo = N > t0l ? N : t0l;
    const int64_t hi = blockIdx.x + 1 == gridDim.x || a.ldy < t0l + kReverbTile ? a.ldy : t0l + kReverbTile;
    for (int64_t j = lo + tid; j < hi; j += kReverbWaves * 64) y[j] = 0.f;
  }
  if (t0l >= nfull) return;
  const int t0 = (int)t0l;  // (the entry point keeps N + M + kReverbTile below 2^31)

  double sum[kReverbAcc][16];
#pragma unroll
  for (int r = 0; r < kReverbAcc; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) sum[r][e] = 0.0;

  const int nblk = (M + 31 + kReverbTapBlock - 1) / kReverbTapBlock;
  for (int blk = 0; blk < nblk; ++blk) {
    const int sb = -31 + blk * kReverbTapBlock;                // the block's first s
    const int ng = (min(kReverbTapBlock, M - sb) + 31) / 32;     // passes of 32 values of s
    // x window of the block: samples n_lo + i, i < 32 (kReverbTile / 32 + ng - 1), at xs[(i >> 5) * 33 + (i & 31)]
    const int n_lo = t0 - sb - 32 * ng + 1;
    const int rows = kReverbTile / 32 + ng - 1;
    if (n_lo + 32 * rows <= 0 || n_lo >= N) continue;  // nothing of the clip in it (the same for every thread)
    __syncthreads();
    for (int i = tid; i < 32 * rows; i += kReverbWaves * 64) {
      const int n = n_lo + i;
      xs[(i >> 5) * kReverbXRow + (i & 31)] = n >= 0 && n < N ? x[n] : 0.f;
    }
    for (int j = tid; j < 32 * ng + 32; j += kReverbWaves * 64) {  // hs[j] = h[sb + j]
      const int m = sb + j;
      hs[j] = m >= 0 && m < M ? h[m] : 0.f;
    }
    __syncthreads();

    // lane (p = lane & 31, half): A[p][s] = x[t0 + 1024 (2 wave + r) + 32 p - s] with s = sb + 32 g + 2 k + half is window index
    // 32 (32 (2 wave + r) + p + ng - 1 - g) + 31 - 2 k - half: row - g, column 31 - 2 k - half
    const float* xa = xs + (32 * kReverbAcc * wave + q + ng - 1) * kReverbXRow + 1 - half;  // column of k = 15
    const float* hb = hs + q + half;
    f32x16 acc[kReverbAcc];
#pragma unroll
    for (int r = 0; r < kReverbAcc; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
    for (int g = 0; g < ng; ++g) {
      float av[kReverbAcc][16], bv[16];  // the pass's fragments first, then its MFMAs
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        bv[k] = hb[2 * k];
#pragma unroll
        for (int r = 0; r < kReverbAcc; ++r) av[r][k] = xa[r * 32 * kReverbXRow + 30 - 2 * k];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int r = 0; r < kReverbAcc; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r][k], bv[k], acc[r], 0, 0, 0);
      xa -= kReverbXRow;
      hb += 32;
    }
#pragma unroll
    for (int r = 0; r < kReverbAcc; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) sum[r][e] += (double)acc[r][e];
  }

  // accumulator register e of lane (q, half) is row (e & 3) + 8 (e >> 2) + 4 half, column q
  unsigned peak = 0;
#pragma unroll
  for (int r = 0; r < kReverbAcc; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t n = t0l + 1024 * (kReverbAcc * wave + r) + 32 * ((e & 3) + 8 * (e >> 2) + 4 * half) + q;
      const float v = (float)sum[r][e];
      if (n < nfull) peak = max(peak, __float_as_uint(v) & 0x7fffffffu);
      if (n < N) y[n] = v;
    }
  if (a.peaks) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) peak = max(peak, (unsigned)__shfl_xor((int)peak, d));
    if (lane == 0 && peak) atomicMax(a.peaks + b, peak);
  }
}

struct ReverbScaleArgs {
  float* y;
  const float* peaks;
  int64_t ldy;
  int len[kReverbMaxClips];
};

// the reference's `if actlev > 0.99: frames = (frames / actlev) * 0.98` on a float32 array: the comparison in double, one correctly
// rounded f32 division and one f32 multiplication per sample
__global__ __launch_bounds__(256) void k_reverb_scale(const ReverbScaleArgs a) {
  const int b = blockIdx.y;
  const float peak = a.peaks[b];
  if (!((double)peak > 0.99)) return;  // a NaN peak leaves the clip as it is
  float* const y = a.y + (int64_t)b * a.ldy;
  const int N = a.len[b];
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) y[n] = (y[n] / peak) * 0.98f;
}

void launch_reverb_rir(const float* x, int B, int64_t ldx, const int64_t* lengths, const float* rirs, int64_t ldr,
                       const int64_t* rir_lengths, const int* rir_index, int R, int normalize, float* y, int64_t ldy, float* peaks,
                       hipStream_t s) {
  if (peaks) VFX_HIP(hipMemsetAsync(peaks, 0, (size_t)B * sizeof(float), s));
  ReverbArgs a{};
  a.rirs = rirs;
  a.ldx = ldx;
  a.ldr = ldr;
  a.ldy = ldy;
  ReverbScaleArgs sa{};
  sa.ldy = ldy;
  for_clip_slices<kReverbMaxClips>(B, [&](int b0, int nb) {
    a.x = slice_rows(x, b0, ldx);
    a.y = slice_rows(y, b0, ldy);
    a.peaks = peaks ? reinterpret_cast<unsigned*>(peaks) + b0 : nullptr;
    const int64_t nmax = narrow_clip_lengths(lengths, b0, nb, a.len);
    std::copy(a.len, a.len + nb, sa.len);
    int64_t nfull = 0;
    for (int i = 0; i < nb; ++i) {
      const int r = rir_index ? rir_index[b0 + i] : (b0 + i) % R;
      a.rir[i] = r;
      a.rir_len[i] = (int)rir_lengths[r];
      nfull = std::max(nfull, lengths[b0 + i] + rir_lengths[r] - 1);
    }
    const dim3 grid((unsigned)((nfull + kReverbTile - 1) / kReverbTile), (unsigned)nb);
    hipLaunchKernelGGL(k_reverb, grid, dim3(kReverbWaves * 64), 0, s, a);
    VFX_HIP(hipGetLastError());
    if (normalize) {
      sa.y = a.y;
      sa.peaks = peaks + b0;
      const dim3 sgrid((unsigned)std::min<int64_t>((nmax + 255) / 256, 256), (unsigned)nb);
      hipLaunchKernelGGL(k_reverb_scale, sgrid, dim3(256), 0, s, sa);
      VFX_HIP(hipGetLastError());
    }
  });
}

}  // namespace vfx
