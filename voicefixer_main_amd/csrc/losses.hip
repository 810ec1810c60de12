// losses.hip -- the validation losses of the training scripts (tools/pytorch/losses.py:192-270 L1_Sp, L1_Log_Sp, nn.L1Loss; val_l of
// models/gsr_voicefixer.py:264-277), forward values only, per clip of a padded batch, gfx950.  Every per-clip sum runs in float64 over
// the clip's own samples or frames, in an order fixed by the clip alone:
//
//   k_pair_stft_l1  one wave per frame walks F consecutive frames of one clip pair, as k_stft_mel does: the front end of stft_wave.h
//                   (reflection at the clip's own end, window, wfft1024, untangle, mag = sqrt(max(re^2 + im^2, eps))) on the est
//                   frame, then on the target frame, and the two sums over the frame's 1025 bins of |se - st| (one float32
//                   subtraction, widened) and |log10(se) - log10(st)| (float64 logarithms) -> ws[(b T + t) 2 + {0, 1}].  No
//                   spectrum reaches memory.  A lane sums its bins lane + 64 m in ascending m (lane 0: bin 1024 last), the wave by
//                   an xor tree: the order does not depend on F or on the grid.
//   k_l1_rows       sum_i |float32(a_i - b_i)| over chunks of kL1Chunk elements of a row, the chunks cut from the row's own start
//                   -> ws[b nchunk + c]: the waveform L1, and the log-mel L1 of val_l over the 128 T_b contiguous floats of a clip
//   k_loss_final    one workgroup per clip: its chunk sums and its frame sums, each taken by index (thread i adds the entries
//                   i, i + 256, ... in ascending order, then the fixed tree of block_sum), divided by the clip's own element count
//
// No float atomics; nothing at or past a clip's length, or a frame at or past its frame count, is read.
#include <cmath>

#include "stft_wave.h"

// (as in stft.hip: the magnitudes here are bit for bit k_stft_mel's, so nothing may fuse differently than there)
#pragma clang fp contract(off)

namespace vfx {

namespace {

constexpr int kWaves = STFT_WAVES;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the 256 threads of a workgroup (fixed order: a wave tree, then the four waves in order); every thread gets it
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[kWaves]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][wave] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
  __syncthreads();
}

}  // namespace

// est, tgt (B, L), pair b = the first lens[b] samples of both rows (NFFT / 2 < lens[b] <= L; lens: device) -> ws[(b T + t) 2 + k],
// t < lens[b] / hop + 1 <= T:  k = 0  sum_bins |float32(se - st)|,  k = 1  sum_bins |log10(se) - log10(st)|; later frames are not written
__global__ __launch_bounds__(STFT_WAVES * 64, 2) void k_pair_stft_l1(const float* __restrict__ est, const float* __restrict__ tgt,
                                                                     int L, int T, const int* __restrict__ lens,
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
  const int b = gw / groups, g = gw - b * groups;
  const int Lb = lens[__builtin_amdgcn_readfirstlane(b)];
  const int Tc = min(T, Lb / hop + 1);
  const int t_begin = g * F, t_end = min(Tc, t_begin + F);
  if (t_begin >= t_end) return;
  const float* xe = est + (int64_t)b * L;
  const float* xt = tgt + (int64_t)b * L;
  float2* zw = zbuf[wave];
  const float2 rtw_lane = rtw[lane];
  float2 xin[16];
  load_frame(xe, Lb, t_begin, hop, lane, xin);
  for (int t = t_begin; t < t_end; ++t) {
    asm volatile("" : "+v"(lane));  // as in the forward kernel: the frame-independent LDS addresses are recomputed per frame
    float2 v[16];
    float se[16], st[16], se_top, st_top;
    window_frame(xin, wl, lane, v);
    load_frame(xt, Lb, t, hop, lane, xin);  // the target frame travels during the est frame's FFT
    frame_magnitudes(v, zw, twl, rtw_lane, lane, eps, se, se_top);
    window_frame(xin, wl, lane, v);
    if (t + 1 < t_end) load_frame(xe, Lb, t + 1, hop, lane, xin);  // ... and the next est frame during the target's
    frame_magnitudes(v, zw, twl, rtw_lane, lane, eps, st, st_top);
    double s_lin = 0.0, s_log = 0.0;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const float d = se[m] - st[m];
      s_lin += (double)fabsf(d);
      s_log += fabs(log10((double)se[m]) - log10((double)st[m]));
    }
    if (lane == 0) {  // bin 1024
      const float d = se_top - st_top;
      s_lin += (double)fabsf(d);
      s_log += fabs(log10((double)se_top) - log10((double)st_top));
    }
    s_lin = wave_sum(s_lin);
    s_log = wave_sum(s_log);
    if (lane == 0) {
      double* w = ws + ((int64_t)b * T + t) * 2;
      w[0] = s_lin;
      w[1] = s_log;
    }
  }
}

// a, b (B, ld), row r = its first n[r] elements (n: device) -> ws[r * nchunk + c] = sum |float32(a_i - b_i)| over the elements
// [c kL1Chunk, min(n[r], (c + 1) kL1Chunk)) of row r; chunks at or past the row's end are not written
__global__ __launch_bounds__(256) void k_l1_rows(const float* __restrict__ a, const float* __restrict__ b, int64_t ld,
                                                 const int* __restrict__ n, int nchunk, double* __restrict__ ws) {
  __shared__ double red[1][kWaves];
  const int r = blockIdx.y, c = blockIdx.x;
  const int64_t len = n[r];
  const int64_t i0 = (int64_t)c * kL1Chunk;
  if (i0 >= len) return;
  const int64_t i1 = min(len, i0 + kL1Chunk);
  const float* pa = a + (int64_t)r * ld;
  const float* pb = b + (int64_t)r * ld;
  double v[1] = {0.0};
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float d = pa[i] - pb[i];
    v[0] += (double)fabsf(d);
  }
  block_sum<1>(v, red);
  if (threadIdx.x == 0) ws[(int64_t)r * nchunk + c] = v[0];
}

// out[b * stride + 0] = (the chunk sums of row b) / counts[b]                           when chunk_ws is given,
// out[b * stride + col + k] = (the frame sums k of clip b) / (frames[b] * nbins), k < 2  when frame_ws is given
__global__ __launch_bounds__(256) void k_loss_final(const double* __restrict__ chunk_ws, int nchunk, const int* __restrict__ counts,
                                                    const double* __restrict__ frame_ws, int T, const int* __restrict__ frames,
                                                    int nbins, int col, double* __restrict__ out, int stride) {
  __shared__ double red[2][kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (chunk_ws) {
    const int64_t count = counts[b];
    const int n = (int)((count + kL1Chunk - 1) / kL1Chunk);
    double v[1] = {0.0};
    for (int c = tid; c < n; c += 256) v[0] += chunk_ws[(int64_t)b * nchunk + c];
    block_sum<1>(v, red);
    if (tid == 0) out[(int64_t)b * stride] = v[0] / (double)count;
  }
  if (frame_ws) {
    const int rows = frames[b];
    double v[2] = {0.0, 0.0};
    for (int t = tid; t < rows; t += 256) {
      const double* w = frame_ws + ((int64_t)b * T + t) * 2;
      v[0] += w[0];
      v[1] += w[1];
    }
    block_sum<2>(v, red);
    if (tid == 0) {
      const double count = (double)rows * (double)nbins;
      out[(int64_t)b * stride + col] = v[0] / count;
      out[(int64_t)b * stride + col + 1] = v[1] / count;
    }
  }
}

void launch_pair_stft_l1(const FrontEndTables& t, const float* est, const float* tgt, int B, int L, int T, const int* lens, int hop,
                         float eps, double* ws, hipStream_t s) {
  const int F = frames_per_group((int64_t)2 * B * T);  // (two transforms per frame)
  const int groups = (T + F - 1) / F;
  const int total = B * groups;
  hipLaunchKernelGGL(k_pair_stft_l1, dim3((total + STFT_WAVES - 1) / STFT_WAVES), dim3(STFT_WAVES * 64), 0, s, est, tgt, L, T, lens,
                     t.window, reinterpret_cast<const float2*>(t.twiddle), reinterpret_cast<const float2*>(t.rtwiddle), hop, eps, F,
                     groups, total, ws);
  VFX_HIP(hipGetLastError());
}

void launch_l1_rows(const float* a, const float* b, int B, int64_t ld, const int* n, int nchunk, double* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_l1_rows, dim3(nchunk, B), dim3(256), 0, s, a, b, ld, n, nchunk, ws);
  VFX_HIP(hipGetLastError());
}

void launch_loss_final(const double* chunk_ws, int nchunk, const int* counts, const double* frame_ws, int T, const int* frames, int nbins,
                       int col, double* out, int stride, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_loss_final, dim3(B), dim3(256), 0, s, chunk_ws, nchunk, counts, frame_ws, T, frames, nbins, col, out, stride);
  VFX_HIP(hipGetLastError());
}

}  // namespace vfx
