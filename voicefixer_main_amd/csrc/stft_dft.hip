// stft_dft.hip -- |STFT| at the prime frame length 743 (hop 160) as a DFT-matrix GEMM on the f32-input MFMA, and its 80-band mel
// projection (gfx950): the front end of the 16 kHz branch of evaluation_proc's AudioMetrics (evaluation_proc/metrics.py:37-51,
// np.abs(librosa.stft(wav, n_fft=743, hop_length=160)) and MelScale(n_mels=80, sample_rate=16000, n_stft=372)).
//
//   sp[b, t, k] = | sum over n < 743 of x_b[reflect(160 t + n - 371)] tab[n][k] |,   tab[n][k] = w[n] e^{-2 pi i (k n mod 743) / 743}
//
// with w the periodic Hann of 743 points, folded into the table on the host (front_end.cpp: float64, rounded to float32 once).  The
// table is (kDftK = 744, 2 x kDftCols = 768) floats: row n = 372 values of w cos, 12 zeros, 372 values of -w sin, 12 zeros; row 743 is
// zeros (K padded to the instruction's step of 2).  It is stored in fragment order (dft_table_index): the 4 + 4 values a lane needs
// for a pass of 8 values of n are 32 consecutive bytes, read as two dwordx4 loads that a half wave covers without a gap.
//
// Work split: a workgroup of four waves owns a strip of kDftStrip = 64 consecutive frames of one clip.  It stages the 743 + 63 x 160
// (+ 1 for the zero row) samples the strip spans ONCE in LDS, straight from the waveform, resolving the reflection at the clip's two
// ends and putting zeros wherever a frame at or past the clip's own count would read; nothing at or past lens[b] is read.  Sample i of
// the strip sits at float i + i / 160: lane p of an A fragment reads frame p, 160 samples after its neighbour, and the skew turns that
// into 161 floats = 33 banks apart.  Wave w computes the bin tiles w, w + 4, w + 8 (32 bins each, 12 tiles = 384 columns), and per
// tile keeps four accumulators of v_mfma_f32_32x32x2_f32: {frames 0-31, frames 32-63} x {re, im}.  The re and im B fragments of a
// k step are the same 32 bins, so the two accumulators of a bin sit in the same lane and register: the magnitude is formed in the
// epilogue without re or im ever reaching memory.
//
// K order: one accumulator chain per element over n = 0 .. 743 ascending, the MFMA's own k-ordered f32 fma chain, started from
// zero.  It is the same for every frame, whatever its place in a strip, the batch or Lmax: a frame's 372 values depend on the clip's
// samples alone, and |re - truth| <= (743 + 1) 2^-24 sum_n |x_n w_n| (one rounding per addition and per table entry).
//
// Mel: after a workgroup barrier the same workgroup projects the rows it has just written (read back through L2 / L1, its own
// stores) onto the packed filterbank, one f32 fma chain per (frame, band) over the band's bins ascending.
//
// Rows t in [frames of the clip, T) of both images are written as zeros, as launch_stft_mel leaves them.
#include "vfx_internal.h"

namespace vfx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kDftWaves = 4;
constexpr int kDftTiles = kDftCols / 32;                             // 12 bin tiles
constexpr int kDftTilesPerWave = kDftTiles / kDftWaves;              // 3
constexpr int kDftSpan = (kDftStrip - 1) * kDftHop + kDftK;          // 10824 samples of a strip (the zero row's included)
constexpr int kDftLds = kDftSpan + (kDftSpan - 1) / kDftHop + 1;     // floats, with the skew of one per hop
static_assert(kDftTiles % kDftWaves == 0 && kDftStrip == 64, "two 32-frame accumulators per wave and bin tile");
static_assert(kDftHop % kDftPass == 0 && kDftK % kDftPass == 0, "a pass stays inside one skew block of kDftHop samples");
static_assert(kDftLds * sizeof(float) <= 64 * 1024, "static LDS");

}  // namespace

// (three workgroups per CU: 3 x 43 KB of LDS, and the registers to match -- the waves of the others cover a wave's table reads)
__global__ __launch_bounds__(kDftWaves * 64, 3) void k_stft_dft(const float* __restrict__ wav, int L, int T,
                                                              const int* __restrict__ lens, const float* __restrict__ tab,
                                                              const float* __restrict__ fb_val, const int* __restrict__ fb_start,
                                                              const int* __restrict__ fb_off, float* sp, float* __restrict__ mel) {
  __shared__ float xs[kDftLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane & 31, half = lane >> 5;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * kDftStrip;
  const int len = lens[b];
  const int frames = dft_frames(len);
  const int tend = min(t0 + kDftStrip, T);  // rows of this strip inside the images
  float* const spb = sp + (int64_t)b * T * kDftBins;
  float* const melb = mel + (int64_t)b * T * kDftMels;

  if (t0 >= frames) {  // nothing of the clip in the strip (the same for every thread): zeros
    for (int i = tid; i < (tend - t0) * kDftBins; i += kDftWaves * 64) spb[(int64_t)t0 * kDftBins + i] = 0.f;
    for (int i = tid; i < (tend - t0) * kDftMels; i += kDftWaves * 64) melb[(int64_t)t0 * kDftMels + i] = 0.f;
    return;
  }

  {  // the strip's samples: padded position 160 t0 + i is sample 160 t0 + i - 371 of the clip, reflected about 0 and len - 1
    const float* const x = wav + (int64_t)b * L;
    const int o0 = t0 * kDftHop - kDftN / 2;
    for (int i = tid; i < kDftSpan; i += kDftWaves * 64) {
      int o = o0 + i;
      if (o < 0) o = -o;
      if (o >= len) o = 2 * (len - 1) - o;
      // (o is outside [0, len) only for frames at or past the clip's count, and for the zero row)
      xs[i + i / kDftHop] = o >= 0 && o < len ? x[o] : 0.f;
    }
  }
  __syncthreads();

  // lane (p = lane & 31, half) of the A fragment of frame tile r, k step k of a pass at n0: sample 160 (32 r + p) + n0 + 2 k + half
  // of the strip, at float 161 (32 r + p) + n0 + n0 / 160 + 2 k + half
  const float* const xa = xs + q * (kDftHop + 1) + half;
#pragma unroll 1
  for (int j = 0; j < kDftTilesPerWave; ++j) {
    const int col = 32 * (wave + kDftWaves * j) + q;             // this lane's bin
    // rows n0 + 2 k + half, k < 4, of the table at this lane's bin: re in tb[0], im in tb[1]
    const float4* tb = reinterpret_cast<const float4*>(tab) + ((int64_t)half * kDftCols + col) * 2;
    f32x16 acc[2][2];  // [frame tile][re, im]
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;
    // The fragments of a pass are read one pass ahead of the MFMAs that use them (b0, b1, av: this pass; c0, c1, cv: the next), so that a wave's own 16 MFMAs
    // cover its table and LDS reads; the last pass reads its own fragments again instead of running past the table.
    float4 b0 = tb[0], b1 = tb[1];
    float av[2][kDftPass / 2];
#pragma unroll
    for (int k = 0; k < kDftPass / 2; ++k)
#pragma unroll
      for (int r = 0; r < 2; ++r) av[r][k] = xa[r * 32 * (kDftHop + 1) + 2 * k];
#pragma unroll 1
    for (int n0 = 0; n0 < kDftK; n0 += kDftPass) {
      const int n1 = n0 + kDftPass < kDftK ? n0 + kDftPass : n0;
      const float4* const tn = tb + (n1 / kDftPass) * (2 * kDftCols * 2);
      const float* const xp = xa + n1 + n1 / kDftHop;
      const float4 c0 = tn[0], c1 = tn[1];
      float cv[2][kDftPass / 2];
#pragma unroll
      for (int k = 0; k < kDftPass / 2; ++k)
#pragma unroll
        for (int r = 0; r < 2; ++r) cv[r][k] = xp[r * 32 * (kDftHop + 1) + 2 * k];
      asm volatile("" ::: "memory");  // the reads stay here, ahead of this pass's MFMAs (the compiler otherwise sinks them to their use)
      const float bre[kDftPass / 2] = {b0.x, b0.y, b0.z, b0.w}, bim[kDftPass / 2] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int k = 0; k < kDftPass / 2; ++k)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          acc[r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r][k], bre[k], acc[r][0], 0, 0, 0);
          acc[r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r][k], bim[k], acc[r][1], 0, 0, 0);
        }
      b0 = c0;
      b1 = c1;
#pragma unroll
      for (int k = 0; k < kDftPass / 2; ++k)
#pragma unroll
        for (int r = 0; r < 2; ++r) av[r][k] = cv[r][k];
    }
    // accumulator register e of lane (q, half) is frame (e & 3) + 8 (e >> 2) + 4 half of its tile, bin `col`
    if (col < kDftBins) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int t = t0 + 32 * r + (e & 3) + 8 * (e >> 2) + 4 * half;
          const float re = acc[r][0][e], im = acc[r][1][e];
          if (t < tend) spb[(int64_t)t * kDftBins + col] = t < frames ? sqrtf(re * re + im * im) : 0.f;
        }
    }
  }

  // the mel rows of the strip, from the rows this workgroup has just stored
  __threadfence_block();
  __syncthreads();
  for (int i = tid; i < (tend - t0) * kDftMels; i += kDftWaves * 64) {
    const int t = t0 + i / kDftMels, m = i % kDftMels;
    float a = 0.f;
    if (t < frames) {
      const float* const row = spb + (int64_t)t * kDftBins + fb_start[m];
      const int o = fb_off[m], n = fb_off[m + 1] - o;
      for (int f = 0; f < n; ++f) a = fmaf(row[f], fb_val[o + f], a);
    }
    melb[(int64_t)t * kDftMels + m] = a;
  }
}

void launch_stft_dft(const Score16kTables& t, const float* wav, int B, int L, int T, const int* lens, float* sp, float* mel,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_stft_dft, dim3((unsigned)((T + kDftStrip - 1) / kDftStrip), (unsigned)B), dim3(kDftWaves * 64), 0, s, wav, L, T,
                     lens, t.table, t.fb_val, t.fb_start, t.fb_off, sp, mel);
  VFX_HIP(hipGetLastError());
}

}  // namespace vfx
