// score.hip -- the spectral and time-domain scores of evaluation_proc's AudioMetrics.evaluation (evaluation_proc/metrics.py:25-106),
// per clip of a padded batch, gfx950.  Every per-clip sum runs in float64 over the clip's own samples, frames or SSIM windows:
//
//   k_sisdr_slabs  <e,t>, <t,t>, <e,e> over slabs of kSisdrSlab samples (a workgroup per (slab, clip))
//   k_score_frames one wave per (clip, frame) reads the est and target rows ONCE and forms the LSD term and the inner products of
//                  the linear rows and of their to_log (log10(max(x, 1e-8))): LSD, non-log SiSpec and log SiSpec in one pass
//   k_ssim_tiles   skimage structural_similarity(win_size=7) on the (T, F) image: a workgroup per 32 x 64 tile of window
//                  positions, the inputs of the tile (38 x 70) in LDS, 7-wide row sums and a 7-row ring of them per thread
//   k_score_final  one workgroup per clip: the slabs, frames and tiles of THAT clip summed in a fixed order, the formulas
//
// and the four mel scores a handler returns for a file with a target (eval_gsr_voicefixer.py:59-64, eval_ssr_unet.py:116-126):
//
//   k_handler_frames  k_score_frames for the GSR handler's operand mix: one wave per (clip, frame) reads the rows of the log10 estimate,
//                     of what the vocoder receives and of the target mel ONCE -- the LSD term of (den, tgt), the inner products of
//                     (lg, to_log(tgt)) and of (from_log(lg), tgt)
//   k_handler_final   one workgroup per clip: its frame sums (of either frame kernel) and its SSIM tiles -> four numbers
//
// Slabs and tiles are cut from the clip's own extent (not from the batch's Lmax or T), and the final sums stop at the clip's own
// count, so a clip's nine numbers do not depend on the batch it is scored in.  No float atomics, no frame at or past a clip's
// `frames` is read.
#include <cfloat>
#include <cmath>

#include "vfx_internal.h"

namespace vfx {

namespace {

constexpr int kWaves = 4;
constexpr int kSsimWin = 7;
constexpr int kSsimHalo = kSsimWin - 1;
constexpr int kSsimRowsPerWave = kSsimTileH / kWaves;          // 8 window rows per thread
constexpr int kSsimInRows = kSsimTileH + kSsimHalo;           // 38
constexpr int kSsimInCols = kSsimTileW + kSsimHalo;           // 70
constexpr int kSsimLdsCols = kSsimInCols + 2;
static_assert(kSsimTileW == 64 && kSsimTileH % kWaves == 0, "one column per lane, the rows split over the waves");

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

// SiSpec (metrics.py:89-95, energy_unify / pow_p_norm of utils.py:81-101): s = <e,g> / (|g|^2 + 1e-8), target s g
__device__ __forceinline__ double sispec_db(double ee, double eg, double gg) {
  const double s = eg / (gg + 1e-8);
  const double pt = s * s * gg;
  const double pn = fmax(ee - 2.0 * s * eg + pt, 0.0);
  return 10.0 * log10(pt / (pn + 1e-12) + 1e-12);
}

}  // namespace

// ws[(b * nslab + s) * 3 + {0, 1, 2}] = <e,t>, <t,t>, <e,e> over samples [s * kSisdrSlab, min(len, (s + 1) * kSisdrSlab)) of clip b;
// slabs at or past the clip's end are not written (the final kernel stops at the clip's own slab count)
__global__ __launch_bounds__(256) void k_sisdr_slabs(const float* __restrict__ est, const float* __restrict__ tgt, int64_t ld,
                                                     const int* __restrict__ lens, int nslab, double* __restrict__ ws) {
  __shared__ double red[3][kWaves];
  const int b = blockIdx.y, s = blockIdx.x;
  const int64_t len = lens[b];
  const int64_t i0 = (int64_t)s * kSisdrSlab;
  if (i0 >= len) return;
  const int64_t i1 = min(len, i0 + kSisdrSlab);
  const float* e = est + (int64_t)b * ld;
  const float* g = tgt + (int64_t)b * ld;
  double v[3] = {0.0, 0.0, 0.0};
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const double ev = e[i], gv = g[i];
    v[0] += ev * gv;   // float x float is exact in double
    v[1] += gv * gv;
    v[2] += ev * ev;
  }
  block_sum<3>(v, red);
  if (threadIdx.x == 0) {
    double* w = ws + ((int64_t)b * nslab + s) * 3;
    w[0] = v[0];
    w[1] = v[1];
    w[2] = v[2];
  }
}

// ws[(b * T + t) * 7 + k], t < frames[b]:  k = 0  sqrt(mean_f log10(g^2 / (e + 1e-12)^2 + 1e-12)^2)  (metrics.py:83-87)
//                                          k = 1..3  <e,e>, <e,g>, <g,g> of the linear rows
//                                          k = 4..6  the same of log10(max(., 1e-8)) of the rows (utils.py:60-61)
__global__ __launch_bounds__(256) void k_score_frames(const float* __restrict__ est, const float* __restrict__ tgt, int T, int F,
                                                      const int* __restrict__ frames, double* __restrict__ ws) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= frames[b]) return;
  const float* e = est + ((int64_t)b * T + t) * F;
  const float* g = tgt + ((int64_t)b * T + t) * F;
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int f = lane; f < F; f += 64) {
    const double ev = e[f], gv = g[f];
    const double d = ev + 1e-12;
    const double l = log10(gv * gv / (d * d) + 1e-12);
    v[0] += l * l;
    v[1] += ev * ev;
    v[2] += ev * gv;
    v[3] += gv * gv;
    const double le = log10(fmax(ev, 1e-8)), lg = log10(fmax(gv, 1e-8));
    v[4] += le * le;
    v[5] += le * lg;
    v[6] += lg * lg;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
    double* w = ws + ((int64_t)b * T + t) * 7;
    w[0] = sqrt(v[0] / (double)F);
#pragma unroll
    for (int k = 1; k < 7; ++k) w[k] = v[k];
  }
}

// ws[b * stride + tile] = sum of the SSIM map over the tile's window positions (skimage.metrics.structural_similarity, 0.18:
// uniform 7 x 7 window, covariances normalised by N - 1, K1 = 0.01, K2 = 0.03, data_range = 2; only windows inside the image)
__global__ __launch_bounds__(256) void k_ssim_tiles(const float* __restrict__ est, const float* __restrict__ tgt, int T, int F,
                                                    const int* __restrict__ frames, int64_t stride, double* __restrict__ ws) {
  __shared__ float xs[kSsimInRows][kSsimLdsCols];
  __shared__ float ys[kSsimInRows][kSsimLdsCols];
  __shared__ double red[1][kWaves];
  const int b = blockIdx.y;
  const int rows = frames[b];
  const int Ho = rows - kSsimHalo, Wo = F - kSsimHalo;  // window positions (rows >= 7 and F >= 7: checked by the callers)
  const int ctiles = (Wo + kSsimTileW - 1) / kSsimTileW;
  const int ntiles = (Ho + kSsimTileH - 1) / kSsimTileH * ctiles;
  const int tile = blockIdx.x;
  if (tile >= ntiles) return;
  const int r0 = tile / ctiles * kSsimTileH, c0 = tile % ctiles * kSsimTileW;
  const float* e = est + (int64_t)b * T * F;
  const float* g = tgt + (int64_t)b * T * F;
  for (int i = threadIdx.x; i < kSsimInRows * kSsimInCols; i += 256) {
    const int r = i / kSsimInCols, c = i - r * kSsimInCols;
    const int gr = r0 + r, gc = c0 + c;
    const bool in = gr < rows && gc < F;
    const int64_t o = (int64_t)gr * F + gc;
    xs[r][c] = in ? e[o] : 0.f;
    ys[r][c] = in ? g[o] : 0.f;
  }
  __syncthreads();
  const int col = threadIdx.x & 63, wr = (threadIdx.x >> 6) * kSsimRowsPerWave;
  const bool col_ok = c0 + col < Wo;
  constexpr double inv_n = 1.0 / (kSsimWin * kSsimWin);
  constexpr double cov_norm = (double)(kSsimWin * kSsimWin) / (kSsimWin * kSsimWin - 1);
  constexpr double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0);
  double hx[kSsimWin], hy[kSsimWin], hxx[kSsimWin], hyy[kSsimWin], hxy[kSsimWin];  // row sums of the last 7 input rows (a ring)
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < kSsimRowsPerWave + kSsimHalo; ++i) {
    const int r = wr + i;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int j = 0; j < kSsimWin; ++j) {
      const double xv = xs[r][col + j], yv = ys[r][col + j];
      sx += xv;
      sy += yv;
      sxx += xv * xv;
      syy += yv * yv;
      sxy += xv * yv;
    }
    const int q = i % kSsimWin;
    hx[q] = sx;
    hy[q] = sy;
    hxx[q] = sxx;
    hyy[q] = syy;
    hxy[q] = sxy;
    if (i >= kSsimHalo) {
      double Sx = 0.0, Sy = 0.0, Sxx = 0.0, Syy = 0.0, Sxy = 0.0;
#pragma unroll
      for (int k = 0; k < kSsimWin; ++k) {
        Sx += hx[k];
        Sy += hy[k];
        Sxx += hxx[k];
        Syy += hyy[k];
        Sxy += hxy[k];
      }
      const double ux = Sx * inv_n, uy = Sy * inv_n;
      const double vx = cov_norm * (Sxx * inv_n - ux * ux);
      const double vy = cov_norm * (Syy * inv_n - uy * uy);
      const double vxy = cov_norm * (Sxy * inv_n - ux * uy);
      const double s = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      if (col_ok && r0 + r - kSsimHalo < Ho) acc += s;
    }
  }
  double v[1] = {acc};
  block_sum<1>(v, red);
  if (threadIdx.x == 0) ws[(int64_t)b * stride + tile] = v[0];
}

// out[b * 9 + k] (AudioMetrics.evaluation's keys in order): sisdr, lsd, non_log_sispec, sispec, ssim, and the four of the mel rows
__global__ __launch_bounds__(256) void k_score_final(ScoreFinalArgs a) {
  __shared__ double red[7][kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  double* out = a.out + (int64_t)b * VFX_N_AUDIO_METRICS;
  const int rows = a.frames ? a.frames[b] : 0;
  if (a.sisdr_ws) {
    // speechmetrics relative/sisdr.py (as recalled; the package is not available to pin it):
    //   a = (eps + <t,e>) / (<t,t> + eps), Sss = |a t|^2, Snn = |e - a t|^2, 10 log10((eps + Sss) / (eps + Snn))
    const int n = (int)((a.lens[b] + kSisdrSlab - 1) / kSisdrSlab);
    double v[3] = {0.0, 0.0, 0.0};
    for (int s = tid; s < n; s += 256) {
      const double* w = a.sisdr_ws + ((int64_t)b * a.nslab + s) * 3;
      v[0] += w[0];
      v[1] += w[1];
      v[2] += w[2];
    }
    block_sum<3>(v, red);
    if (tid == 0) {
      const double eps = DBL_EPSILON, et = v[0], tt = v[1], ee = v[2];
      const double al = (eps + et) / (tt + eps);
      const double sss = al * al * tt;
      const double snn = fmax(ee - 2.0 * al * et + al * al * tt, 0.0);
      out[0] = 10.0 * log10((eps + sss) / (eps + snn));
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (a.frames_ws[m]) {
      double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int t = tid; t < rows; t += 256) {
        const double* w = a.frames_ws[m] + ((int64_t)b * a.T + t) * 7;
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] += w[k];
      }
      block_sum<7>(v, red);
      if (tid == 0) {
        out[1 + 4 * m] = v[0] / (double)rows;
        out[2 + 4 * m] = sispec_db(v[1], v[2], v[3]);
        out[3 + 4 * m] = sispec_db(v[4], v[5], v[6]);
      }
    }
    if (a.ssim_ws[m]) {
      const int Ho = rows - kSsimHalo, Wo = a.F[m] - kSsimHalo;
      const int n = (Ho + kSsimTileH - 1) / kSsimTileH * ((Wo + kSsimTileW - 1) / kSsimTileW);
      double v[1] = {0.0};
      for (int i = tid; i < n; i += 256) v[0] += a.ssim_ws[m][(int64_t)b * a.ssim_stride[m] + i];
      block_sum<1>(v, red);
      if (tid == 0) out[4 + 4 * m] = v[0] / ((double)Ho * (double)Wo);
    }
  }
}

// ws[(b * T + t) * 7 + k], t < frames[b], of three (B, T, 128) images -- lg the log10 estimate, den what the vocoder receives, tgt the
// target's linear mel (eval_gsr_voicefixer.py:59-64):
//   k = 0     sqrt(mean_f log10(tgt^2 / (den + 1e-12)^2 + 1e-12)^2)            the LSD term of (den, tgt)
//   k = 1..3  <e,e>, <e,g>, <g,g> of e = lg, g = log10(max(tgt, 1e-8))         mel-sispec
//   k = 4..6  the same of e = from_log(lg) (float32, k_from_log's value), g = tgt  mel-non-log-sispec (before unify_energy)
__global__ __launch_bounds__(256) void k_handler_frames(const float* __restrict__ lg, const float* __restrict__ den,
                                                        const float* __restrict__ tgt, int T, const int* __restrict__ frames,
                                                        double* __restrict__ ws) {
  constexpr int F = 128;
  const int b = blockIdx.y;
  const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= frames[b]) return;
  const int64_t row = ((int64_t)b * T + t) * F;
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int f = lane; f < F; f += 64) {
    const float lf = lg[row + f];
    const double gv = tgt[row + f];
    const double d = (double)den[row + f] + 1e-12;
    const double l = log10(gv * gv / (d * d) + 1e-12);
    v[0] += l * l;
    const double le = lf, lt = log10(fmax(gv, 1e-8));
    v[1] += le * le;
    v[2] += le * lt;
    v[3] += lt * lt;
    const double ev = from_log_value(lf);
    v[4] += ev * ev;
    v[5] += ev * gv;
    v[6] += gv * gv;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
    double* w = ws + ((int64_t)b * T + t) * 7;
    w[0] = sqrt(v[0] / (double)F);
#pragma unroll
    for (int k = 1; k < 7; ++k) w[k] = v[k];
  }
}

// out[b * 4 + {0, 1, 2, 3}] = mel-lsd, mel-sispec, mel-non-log-sispec, mel-ssim of clip b from its frames_ws rows ([B][T][7]) and its
// SSIM tile sums ([B][ssim_stride]), summed in an order fixed by its own frame count.  log_first: columns 1..3 of frames_ws hold the
// log-domain inner products (k_handler_frames); 0: the linear ones (k_score_frames)
__global__ __launch_bounds__(256) void k_handler_final(const double* __restrict__ frames_ws, int T, const int* __restrict__ frames,
                                                       const double* __restrict__ ssim_ws, int64_t ssim_stride, int F, int log_first,
                                                       double* __restrict__ out) {
  __shared__ double red[7][kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int rows = frames[b];
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = tid; t < rows; t += 256) {
    const double* w = frames_ws + ((int64_t)b * T + t) * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] += w[k];
  }
  block_sum<7>(v, red);
  const int Ho = rows - kSsimHalo, Wo = F - kSsimHalo;
  const int n = (Ho + kSsimTileH - 1) / kSsimTileH * ((Wo + kSsimTileW - 1) / kSsimTileW);
  double q[1] = {0.0};
  for (int i = tid; i < n; i += 256) q[0] += ssim_ws[(int64_t)b * ssim_stride + i];
  block_sum<1>(q, red);
  if (tid == 0) {
    double* o = out + (int64_t)b * VFX_N_HANDLER_METRICS;
    const double a = sispec_db(v[1], v[2], v[3]), c = sispec_db(v[4], v[5], v[6]);
    o[0] = v[0] / (double)rows;
    o[1] = log_first ? a : c;
    o[2] = log_first ? c : a;
    o[3] = q[0] / ((double)Ho * (double)Wo);
  }
}

void launch_sisdr_slabs(const float* est, const float* tgt, int B, int64_t ld, const int* lens, int nslab, double* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_sisdr_slabs, dim3(nslab, B), dim3(256), 0, s, est, tgt, ld, lens, nslab, ws);
  VFX_HIP(hipGetLastError());
}

void launch_score_frames(const float* est, const float* tgt, int B, int T, int F, const int* frames, double* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_score_frames, dim3((T + kWaves - 1) / kWaves, B), dim3(256), 0, s, est, tgt, T, F, frames, ws);
  VFX_HIP(hipGetLastError());
}

void launch_ssim_tiles(const float* est, const float* tgt, int B, int T, int F, const int* frames, double* ws, hipStream_t s) {
  const int64_t n = ssim_tiles(T, F);
  hipLaunchKernelGGL(k_ssim_tiles, dim3((unsigned)n, B), dim3(256), 0, s, est, tgt, T, F, frames, n, ws);
  VFX_HIP(hipGetLastError());
}

void launch_score_final(const ScoreFinalArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_score_final, dim3(B), dim3(256), 0, s, a);
  VFX_HIP(hipGetLastError());
}

static size_t handler_frames_bytes(int B, int T) { return ((size_t)B * T * 7 * sizeof(double) + 255) / 256 * 256; }

size_t handler_metrics_ws_bytes(int B, int T) { return handler_frames_bytes(B, T) + (size_t)B * ssim_tiles(T, 128) * sizeof(double); }

static void launch_handler_tail(const float* img, const float* tgt, int B, int T, const int* frames, char* ws, int log_first, double* out,
                                hipStream_t s) {
  double* const fr = reinterpret_cast<double*>(ws);
  double* const ss = reinterpret_cast<double*>(ws + handler_frames_bytes(B, T));
  launch_ssim_tiles(img, tgt, B, T, 128, frames, ss, s);
  hipLaunchKernelGGL(k_handler_final, dim3(B), dim3(256), 0, s, fr, T, frames, ss, (int64_t)ssim_tiles(T, 128), 128, log_first, out);
  VFX_HIP(hipGetLastError());
}

void launch_handler_metrics(const float* lg, const float* den, const float* tgt, int B, int T, const int* frames, char* ws, double* out,
                            hipStream_t s) {
  hipLaunchKernelGGL(k_handler_frames, dim3((T + kWaves - 1) / kWaves, B), dim3(256), 0, s, lg, den, tgt, T, frames,
                     reinterpret_cast<double*>(ws));
  VFX_HIP(hipGetLastError());
  launch_handler_tail(den, tgt, B, T, frames, ws, 1, out, s);
}

void launch_mel_metrics(const float* est, const float* tgt, int B, int T, const int* frames, char* ws, double* out, hipStream_t s) {
  launch_score_frames(est, tgt, B, T, 128, frames, reinterpret_cast<double*>(ws), s);
  launch_handler_tail(est, tgt, B, T, frames, ws, 0, out, s);
}

}  // namespace vfx
