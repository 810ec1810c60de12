// band.hip -- the bandwidth detector in front of the reference's restoration handlers (tools/utils.py:33-44 load_wav_energy: the
// frequency bin below which `threshold` of a clip's log-spectral energy lies), per clip of a padded batch, gfx950.
//
//   k_band_energy  one wave per frame walks kBandFrames consecutive frames of one clip, as k_pair_stft_l1 does: the front end of
//                  stft_wave.h at the call's hop (reflection at the clip's own end, window, wfft1024, untangle, the UNCLAMPED float32
//                  magnitude sqrt(re^2 + im^2)), then log10((double)mag + 1) added to the wave's 1025 per-bin sums in registers -- a
//                  lane keeps its bins lane + 64 m, lane 0 bin 1024 as well -- in ascending t -> ws[(b groups + g) 1025 + k].  The next
//                  frame travels during the transform.  No spectrum reaches memory.  The number of frames a wave walks is a constant:
//                  which frames a partial sum holds is fixed by the clip's own length and the hop.
//   k_band_cut     one workgroup per clip: e[k] = its group partials in ascending g (-> energy when asked), the exclusive prefix
//                  P[k] = sum_{j<k} e[j] in ascending k (the loop of utils.py:38-39; total = P[1024], bin 1024 never counts), and
//                  cut_bin = the first k that does not have P[k] < total * threshold (utils.py:41-43), 1024 when there is none.
//
// Every sum is float64 in an order fixed by the clip alone.  No float atomics; nothing at or past a clip's length, or a group at or past
// its group count, is read.
#include <cmath>

#include "clip_batch.h"
#include "stft_wave.h"

// (as in stft.hip: the magnitudes are the shared front end's, nothing may fuse differently than there)
#pragma clang fp contract(off)

namespace vfx {

namespace {

struct BandArgs {
  int len[kBandMaxClips];  // samples per clip of the slice
};

}  // namespace

// wav (nb, ld), clip b = its first a.len[b] samples (NFFT / 2 < len <= ld) -> ws[(b groups + g) 1025 + k], g < ceil(T_b / kBandFrames),
// T_b = len / hop + 1: the sum over the frames [g kBandFrames, min(T_b, (g + 1) kBandFrames)) of log10(|X_t[k]| + 1); later groups are
// not written
__global__ __launch_bounds__(STFT_WAVES * 64, 2) void k_band_energy(const float* __restrict__ wav, int64_t ld, const BandArgs a,
                                                                    const float* __restrict__ window, const float2* __restrict__ tw,
                                                                    const float2* __restrict__ rtw, int hop, int groups,
                                                                    int total_groups, double* __restrict__ ws) {
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
  const int gw = blockIdx.x * STFT_WAVES + wave;  // this wave's group of kBandFrames consecutive frames of one clip
  if (gw >= total_groups) return;
  const int b = gw / groups, g = gw - b * groups;
  const int Lb = a.len[b];
  const int Tb = Lb / hop + 1;
  const int t_begin = g * kBandFrames, t_end = min(Tb, t_begin + kBandFrames);
  if (t_begin >= t_end) return;
  const float* x = wav + (int64_t)b * ld;
  float2* zw = zbuf[wave];
  const float2 rtw_lane = rtw[lane];
  double acc[16], acc_top = 0.0;  // bins lane + 64 m, and bin 1024 (lane 0's; the other lanes add log10(1) = 0)
#pragma unroll
  for (int m = 0; m < 16; ++m) acc[m] = 0.0;
  float2 xin[16];
  load_frame(x, Lb, t_begin, hop, lane, xin);
  for (int t = t_begin; t < t_end; ++t) {
    asm volatile("" : "+v"(lane));  // as in the forward kernel: the frame-independent LDS addresses are recomputed per frame
    float2 v[16];
    float mag[16], top;
    window_frame(xin, wl, lane, v);
    if (t + 1 < t_end) load_frame(x, Lb, t + 1, hop, lane, xin);  // the next frame travels during this one's FFT
    frame_magnitudes(v, zw, twl, rtw_lane, lane, 0.f, mag, top);
#pragma unroll
    for (int m = 0; m < 16; ++m) acc[m] += log10((double)mag[m] + 1.0);
    acc_top += log10((double)top + 1.0);
  }
  double* w = ws + ((int64_t)b * groups + g) * NBINS;
#pragma unroll
  for (int m = 0; m < 16; ++m) w[lane + 64 * m] = acc[m];
  if (lane == 0) w[NC] = acc_top;
}

// ws as k_band_energy leaves it -> energy[b][k] (when given) and cut[b]
__global__ __launch_bounds__(256) void k_band_cut(const double* __restrict__ ws, const BandArgs a, int hop, int groups, double threshold,
                                                  double* __restrict__ energy, int* __restrict__ cut) {
  __shared__ double e[NBINS], P[NBINS];
  __shared__ int first;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int gb = (a.len[b] / hop + 1 + kBandFrames - 1) / kBandFrames;  // the clip's own groups
  const double* w = ws + (int64_t)b * groups * NBINS;
  for (int k = tid; k < NBINS; k += 256) {
    double s = 0.0;
#pragma unroll 8
    for (int g = 0; g < gb; ++g) s += w[(int64_t)g * NBINS + k];  // (eight loads in flight; the additions stay in ascending g)
    e[k] = s;
    if (energy) energy[(int64_t)b * NBINS + k] = s;
  }
  if (tid == 0) first = NBINS - 1;
  __syncthreads();
  if (tid == 0) {  // one chain of 1025 additions: the order is the definition
    double p = 0.0;
#pragma unroll 8
    for (int k = 0; k < NBINS; ++k) {
      P[k] = p;
      p += e[k];
    }
  }
  __syncthreads();
  const double level = P[NBINS - 1] * threshold;
  for (int k = tid; k < NBINS; k += 256)
    if (!(P[k] < level)) atomicMin(&first, k);  // (an integer in LDS: the smallest k, whatever the order)
  __syncthreads();
  if (tid == 0) cut[b] = first;
}

void launch_band_energy(const FrontEndTables& t, const float* wav, int nb, int64_t ld, const int* len, int hop, double threshold,
                        int groups, double* ws, double* energy, int* cut_bin, hipStream_t s) {
  BandArgs a;
  for (int i = 0; i < kBandMaxClips; ++i) a.len[i] = i < nb ? len[i] : 0;
  const int total = nb * groups;
  hipLaunchKernelGGL(k_band_energy, dim3((total + STFT_WAVES - 1) / STFT_WAVES), dim3(STFT_WAVES * 64), 0, s, wav, ld, a, t.window,
                     reinterpret_cast<const float2*>(t.twiddle), reinterpret_cast<const float2*>(t.rtwiddle), hop, groups, total, ws);
  VFX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_band_cut, dim3(nb), dim3(256), 0, s, ws, a, hop, groups, threshold, energy, cut_bin);
  VFX_HIP(hipGetLastError());
}

}  // namespace vfx
