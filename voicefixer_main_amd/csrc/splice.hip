// splice.hip -- the level match of the splice (vfx_band_power): the power of two clips in a band of STFT bins, per clip pair of a
// padded batch, gfx950.  What the splice's gain sqrt(p_in / p_out) is made of: the band just under the seam, where the input and the
// restored clip both carry signal (the idea of amp_to_original_f, tools/utils.py:50-55, with the band chosen per clip).
//
//   k_pair_band_power   one wave per frame walks F consecutive frames of one clip pair, as k_pair_stft_l1 does: the front end of
//                       stft_wave.h (reflection at the clip's own end, window, wfft1024, untangle, mag = sqrt(max(re^2 + im^2, 1e-8)))
//                       on the frame of a, then of b, and for each the sum over the bins lo <= k < hi of (double)mag^2 (the square of a
//                       float32 is exact in float64) -> ws[(b T + t) 2 + {0, 1}].  No spectrum reaches memory.  A lane sums its bins
//                       lane + 64 m in ascending m (lane 0: bin 1024 last), the wave by an xor tree: the order does not depend on F or
//                       on the grid.
//   k_band_power_final  one workgroup per pair: its frame sums taken by index (thread i adds the frames i, i + 256, ... in ascending
//                       order, then the fixed tree of block_sum, as k_loss_final does) -> out[b][0..1].
//
// No float atomics; nothing at or past a clip's length, or a frame at or past its frame count, is read.
#include "stft_wave.h"

// (as in stft.hip: the magnitudes here are bit for bit k_stft_mel's, so nothing may fuse differently than there)
#pragma clang fp contract(off)

namespace vfx {

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace

// a, b (B, L), pair p = the first lens[p] samples of both rows (NFFT / 2 < lens[p] <= L; lens, lo, hi: device) -> ws[(p T + t) 2 + k],
// t < lens[p] / hop + 1 <= T:  k = 0  sum_{lo[p] <= j < hi[p]} |A_t[j]|^2,  k = 1  the same of b; later frames are not written
__global__ __launch_bounds__(STFT_WAVES * 64, 2) void k_pair_band_power(const float* __restrict__ a, const float* __restrict__ b, int L,
                                                                        int T, const int* __restrict__ lens,
                                                                        const int* __restrict__ lo, const int* __restrict__ hi,
                                                                        const float* __restrict__ window,
                                                                        const float2* __restrict__ tw,
                                                                        const float2* __restrict__ rtw, int hop, float eps, int F,
                                                                        int groups, int total_groups, double* __restrict__ ws) {
  __shared__ float2 twl[NC];
  __shared__ float2 wl[NC];  // the window, as pairs (w[2n], w[2n+1])
  __shared__ float2 zbuf[STFT_WAVES][ZP];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int lane = tid & 63;
#pragma unroll
  for (int r = 0; r < NC / (STFT_WAVES * 64); ++r) {
    twl[tid + r * STFT_WAVES * 64] = tw[tid + r * STFT_WAVES * 64];
    wl[tid + r * STFT_WAVES * 64] = *reinterpret_cast<const float2*>(window + 2 * (tid + r * STFT_WAVES * 64));
  }
  __syncthreads();  // the only block barrier: from here on the waves are independent
  const int gw = blockIdx.x * STFT_WAVES + wave;  // this wave's group of F consecutive frames of one pair
  if (gw >= total_groups) return;
  const int p = __builtin_amdgcn_readfirstlane(gw / groups), g = gw - p * groups;
  const int Lp = lens[p], k_lo = lo[p], k_hi = hi[p];
  const int Tc = min(T, Lp / hop + 1);
  const int t_begin = g * F, t_end = min(Tc, t_begin + F);
  if (t_begin >= t_end) return;
  const float* xa = a + (int64_t)p * L;
  const float* xb = b + (int64_t)p * L;
  float2* zw = zbuf[wave];
  const float2 rtw_lane = rtw[lane];
  auto band_sum = [&](const float (&mag)[16], float top) __attribute__((always_inline)) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int k = lane + 64 * m;
      const double v = (double)mag[m];
      if (k >= k_lo && k < k_hi) s += v * v;
    }
    if (lane == 0 && NC >= k_lo && NC < k_hi) s += (double)top * (double)top;  // bin 1024
    return wave_sum(s);
  };
  float2 xin[16];
  load_frame(xa, Lp, t_begin, hop, lane, xin);
  for (int t = t_begin; t < t_end; ++t) {
    asm volatile("" : "+v"(lane));  // as in the forward kernel: the frame-independent LDS addresses are recomputed per frame
    float2 v[16];
    float mag[16], top;
    window_frame(xin, wl, lane, v);
    load_frame(xb, Lp, t, hop, lane, xin);  // the frame of b travels during the transform of a's
    frame_magnitudes(v, zw, twl, rtw_lane, lane, eps, mag, top);
    const double pa = band_sum(mag, top);
    window_frame(xin, wl, lane, v);
    if (t + 1 < t_end) load_frame(xa, Lp, t + 1, hop, lane, xin);  // ... and the next frame of a during b's
    frame_magnitudes(v, zw, twl, rtw_lane, lane, eps, mag, top);
    const double pb = band_sum(mag, top);
    if (lane == 0) {
      double* w = ws + ((int64_t)p * T + t) * 2;
      w[0] = pa;
      w[1] = pb;
    }
  }
}

// out[p * 2 + k] = the frame sums k of pair p over its frames[p] frames
__global__ __launch_bounds__(256) void k_band_power_final(const double* __restrict__ ws, int T, const int* __restrict__ frames,
                                                          double* __restrict__ out) {
  __shared__ double red[2][STFT_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rows = frames[p];
  double v[2] = {0.0, 0.0};
  for (int t = tid; t < rows; t += 256) {
    const double* w = ws + ((int64_t)p * T + t) * 2;
    v[0] += w[0];
    v[1] += w[1];
  }
  // (k_loss_final's block_sum: a wave tree, then the four waves in order)
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    v[k] = wave_sum(v[k]);
    if (lane == 0) red[k][wave] = v[k];
  }
  __syncthreads();
  if (tid < 2) out[(int64_t)p * 2 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

void launch_pair_band_power(const FrontEndTables& t, const float* a, const float* b, int B, int L, int T, const int* lens, const int* lo,
                            const int* hi, const int* frames, int hop, float eps, double* ws, double* out, hipStream_t s) {
  const int F = frames_per_group((int64_t)2 * B * T);  // (two transforms per frame)
  const int groups = (T + F - 1) / F;
  const int total = B * groups;
  hipLaunchKernelGGL(k_pair_band_power, dim3((total + STFT_WAVES - 1) / STFT_WAVES), dim3(STFT_WAVES * 64), 0, s, a, b, L, T, lens, lo,
                     hi, t.window, reinterpret_cast<const float2*>(t.twiddle), reinterpret_cast<const float2*>(t.rtwiddle), hop, eps, F,
                     groups, total, ws);
  VFX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_band_power_final, dim3(B), dim3(256), 0, s, ws, T, frames, out);
  VFX_HIP(hipGetLastError());
}

}  // namespace vfx
