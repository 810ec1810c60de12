// bsseval.hip -- BSS Eval v4 "images" SDR, ISR and SAR (Vincent, Gribonval, Fevotte, IEEE TASLP 2006; the SiSEC 2018 form, restated
// from the definition in include/vfx.h -- not pinned against museval), one source, one channel, one window over the whole file, per
// clip of a padded batch, gfx950.  Float32 clips in, float64 from the first multiply on; the matrix work runs on
// v_mfma_f64_16x16x4_f64, whose result layout is its own: lane l, register g holds D[row = (l >> 4) + 4 g][col = l & 15].
// r = target, e = est, n = the clip's samples, L = flen (a multiple of 16, <= 512).
//
//   k_bss_corr     a[k] = sum_t r[t] r[t + k] and d[k] = sum_t e[t] r[t - k], k < L, as ONE Hankel GEMM with time as K:
//                  (A B)[q][p] = sum_t r[t - q] x[t + 16 p + 256 h] = lag 256 h + 16 p + q of (x, r), x = r and x = e, A[q][t] = r[t - q]:
//                  four accumulators of 256 lags that share the A fragments.  A workgroup per (slab of kSlab values of t, clip); a
//                  tile of 512 t is staged in LDS as doubles from 16-byte sample groups, its K steps split over the four waves, the
//                  waves' accumulators added in wave order
//   k_bss_lags     one workgroup per clip: the slabs of each lag summed in ascending order
//   k_bss_solve    one workgroup per clip: (toeplitz(a) + 2^-52 I) c = d by the Levinson recursion in LDS, L = 16 .. 512 in one path
//   k_bss_project  P = c * r in direct form, y[t0 + 16 p + q] = sum_s A[p][s] B[s][q], A[p][s] = r[t0 + 16 p - s], B[s][q] = c[q + s],
//                  s = -16 .. L - 1; 256 outputs per wave and tile.  The epilogue adds each output's terms of the energies
//                  sum r^2, (e - r)^2, (P - r)^2, P^2, (e - P)^2, e^2 over t < n + L - 1; P is stored only for the test stage.
//                  A workgroup per (slab of kSlab outputs, clip)
//   k_bss_final    one workgroup per clip: the slabs of each energy in ascending order, then the three scores
//
// Slabs are cut from the clip's own extent and every sum runs in an order fixed by the clip alone: a clip's scores do not depend on
// the batch, on Lmax, nor on what lies at or past its length in its row -- nothing there is read.  No float atomics.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "clip_batch.h"
#include "vfx_internal.h"

namespace vfx {

namespace {

constexpr int kWaves = 4;
constexpr int kSlab = VFX_BSSEVAL_SLAB;
constexpr int kF = kBssMaxFlen;              // row length of the lag and filter arrays of the workspace
constexpr int kCorrTile = 512;               // values of t per staging of k_bss_corr, 128 per wave
constexpr int kProjWave = 256;               // outputs per wave and tile of k_bss_project: one accumulator
constexpr int kProjTile = kWaves * kProjWave;
constexpr int kEnergies = 6;                 // the five of the definition and sum e^2 (the silent-est rule)
static_assert(kSlab % kCorrTile == 0 && kSlab % kProjTile == 0, "whole tiles per slab");
static_assert(kF == 512, "two accumulators of 256 lags per signal");

typedef double d4 __attribute__((ext_vector_type(4)));

// LDS rows are read 16 doubles apart by the 16 lanes of a fragment column: two doubles of padding per 16 put the 32 lanes of a
// half wave on 32 different bank pairs
__host__ __device__ constexpr int pad16(int j) { return j + 2 * (j >> 4); }
constexpr int padded_len(int n) { return pad16(n + 15); }

struct BssWs {
  double* lagp;  // [n][ns][2][kF]        per-slab lag sums: a, d
  double* ad;    // [n][2][kF]            a, d
  double* c;     // [n][kF]               the filter
  double* enp;   // [n][nso][kEnergies]   per-slab energies
  double* en;    // [n][kEnergies]
  int ns, nso;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// dst[pad16(i)] = row[j0 + i], i < count (a multiple of 4; j0 a multiple of 4), zeros outside [0, n)
__device__ __forceinline__ void stage_samples(double* dst, int count, const float* row, bool vec, int64_t j0, int64_t n) {
  for (int g = threadIdx.x; g < count / 4; g += 256) {
    const int64_t j = j0 + 4 * g;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (j >= 0 && j < n) clip_load(row, vec, j, n, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[pad16(4 * g + e)] = (double)v[e];
  }
}

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

}  // namespace

__global__ __launch_bounds__(256) void k_bss_corr(const float* __restrict__ est, const float* __restrict__ tgt, int64_t ld,
                                                  const int* __restrict__ lens, int flen, BssWs ws) {
  constexpr int kRA = 16 + kCorrTile + 512, kEB = kCorrTile + 512;   // r[tt - 16 ..), e[tt ..): the tile and 511 samples of lag
  __shared__ double rA[padded_len(kRA)], eB[padded_len(kEB)], red[kWaves][4][256];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kk = lane >> 4;
  const int64_t n = lens[b];
  const int64_t t0 = (int64_t)s * kSlab;
  if (t0 >= n) return;
  const int64_t t1 = min(n, t0 + kSlab);
  const float* e = est + (int64_t)b * ld;
  const float* r = tgt + (int64_t)b * ld;
  const bool vece = clip_aligned(e), vecr = clip_aligned(r);
  const bool two = flen > 256;
  const d4 zero = {0.0, 0.0, 0.0, 0.0};
  d4 acc[4] = {zero, zero, zero, zero};  // a: lags 0..255, 256..511; d: the same
  for (int64_t tt = t0; tt < t1; tt += kCorrTile) {
    __syncthreads();
    stage_samples(rA, kRA, r, vecr, tt - 16, n);
    stage_samples(eB, kEB, e, vece, tt, n);
    __syncthreads();
    const int w0 = (kCorrTile / kWaves) * wave;
    if (tt + w0 >= t1) continue;  // (wave-uniform) every product of these K steps has a factor at or past n: zero
    for (int k = 0; k < kCorrTile / kWaves; k += 4) {
      const int o = w0 + k + kk;  // t = tt + o
      const double av = rA[pad16(16 + o - i)];
      acc[0] = mfma(av, rA[pad16(16 + o + 16 * i)], acc[0]);
      acc[2] = mfma(av, eB[pad16(o + 16 * i)], acc[2]);
      if (two) {
        acc[1] = mfma(av, rA[pad16(16 + o + 16 * i + 256)], acc[1]);
        acc[3] = mfma(av, eB[pad16(o + 16 * i + 256)], acc[3]);
      }
    }
  }
  // lag 16 p + q of an accumulator sits at row q = (lane >> 4) + 4 g, column p = lane & 15
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int g = 0; g < 4; ++g) red[wave][a][16 * i + kk + 4 * g] = acc[a][g];
  __syncthreads();
  double* out = ws.lagp + ((int64_t)b * ws.ns + s) * 2 * kF;
  for (int idx = tid; idx < 4 * 256; idx += 256) {
    const int a = idx >> 8, l = idx & 255;
    out[(a >> 1) * kF + (a & 1) * 256 + l] = ((red[0][a][l] + red[1][a][l]) + red[2][a][l]) + red[3][a][l];
  }
}

__global__ __launch_bounds__(256) void k_bss_lags(const int* __restrict__ lens, int flen, BssWs ws) {
  const int b = blockIdx.x;
  const int nsl = (int)(((int64_t)lens[b] + kSlab - 1) / kSlab);
  for (int idx = threadIdx.x; idx < 2 * flen; idx += 256) {
    const int sig = idx / flen, lag = idx - sig * flen;
    const double* p = ws.lagp + ((int64_t)b * ws.ns * 2 + sig) * kF + lag;
    double v = 0.0;
    for (int s = 0; s < nsl; ++s) v += p[(int64_t)s * 2 * kF];
    ws.ad[((int64_t)b * 2 + sig) * kF + lag] = v;
  }
}

// Levinson: with f the first column of the inverse of the leading m x m block G_m (so G_m f = e_1, and by symmetry G_m rev(f) = e_m)
// and x the solution of G_m x = d[:m], the step to m + 1 needs ef = sum_i a[m - i] f[i] and ex = sum_i a[m - i] x[i]:
//   f' = ([f, 0] - ef [0, rev(f)]) / (1 - ef^2),   x' = [x, 0] + (d[m] - ex) rev(f')
__global__ __launch_bounds__(256) void k_bss_solve(int flen, BssWs ws) {
  __shared__ double a[kF], d[kF], f[2][kF], x[kF], red[2][kWaves][2];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < flen; i += 256) {
    a[i] = ws.ad[((int64_t)b * 2 + 0) * kF + i] + (i == 0 ? DBL_EPSILON : 0.0);
    d[i] = ws.ad[((int64_t)b * 2 + 1) * kF + i];
  }
  __syncthreads();
  if (tid == 0) {
    f[0][0] = 1.0 / a[0];
    x[0] = d[0] / a[0];
  }
  __syncthreads();
  int cur = 0;
  for (int m = 1; m < flen; ++m) {
    double pf = 0.0, px = 0.0;
    for (int i = tid; i < m; i += 256) {
      const double am = a[m - i];
      pf += am * f[cur][i];
      px += am * x[i];
    }
    pf = wave_sum(pf);
    px = wave_sum(px);
    if (lane == 0) {
      red[m & 1][wave][0] = pf;
      red[m & 1][wave][1] = px;
    }
    __syncthreads();
    const double ef = ((red[m & 1][0][0] + red[m & 1][1][0]) + red[m & 1][2][0]) + red[m & 1][3][0];
    const double ex = ((red[m & 1][0][1] + red[m & 1][1][1]) + red[m & 1][2][1]) + red[m & 1][3][1];
    const double inv = 1.0 / (1.0 - ef * ef);
    for (int i = tid; i <= m; i += 256) {
      const double fi = i < m ? f[cur][i] : 0.0, bi = i >= 1 ? f[cur][m - i] : 0.0;
      f[cur ^ 1][i] = (fi - ef * bi) * inv;
    }
    __syncthreads();
    const double g = d[m] - ex;
    for (int i = tid; i <= m; i += 256) x[i] = (i < m ? x[i] : 0.0) + g * f[cur ^ 1][m - i];
    cur ^= 1;
  }
  __syncthreads();
  for (int i = tid; i < flen; i += 256) ws.c[(int64_t)b * kF + i] = x[i];
}

__global__ __launch_bounds__(256) void k_bss_project(const float* __restrict__ est, const float* __restrict__ tgt, int64_t ld,
                                                     const int* __restrict__ lens, int flen, BssWs ws, double* __restrict__ P,
                                                     int64_t ldp) {
  constexpr int kRP = 512 + kProjTile + 16;  // r[tt - 512 ..): 511 samples of history, the tile, the 16 of s < 0
  __shared__ double rP[padded_len(kRP)], cp[kF + 32], red[kEnergies][kWaves];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kk = lane >> 4;
  const int64_t n = lens[b];
  const int64_t nout = n + flen - 1;
  const int64_t t0 = (int64_t)s * kSlab;
  if (t0 >= nout) return;
  const int64_t t1 = min(nout, t0 + kSlab);
  const float* e = est + (int64_t)b * ld;
  const float* r = tgt + (int64_t)b * ld;
  const bool vecr = clip_aligned(r);
  for (int j = tid; j < kF + 32; j += 256) cp[j] = (j >= 16 && j < 16 + flen) ? ws.c[(int64_t)b * kF + j - 16] : 0.0;  // c[j - 16]
  double en[kEnergies] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int ksteps = (flen + 16) / 4;
  const d4 zero = {0.0, 0.0, 0.0, 0.0};
  for (int64_t tt = t0; tt < t1; tt += kProjTile) {
    __syncthreads();
    stage_samples(rP, kRP, r, vecr, tt - 512, n);
    __syncthreads();
    const int64_t tw = tt + kProjWave * wave;
    if (tw >= t1) continue;  // (wave-uniform)
    d4 acc = zero;
    for (int ks = 0; ks < ksteps; ++ks) {
      const int sv = 4 * ks + kk - 16;  // s
      acc = mfma(rP[pad16(512 + kProjWave * wave + 16 * i - sv)], cp[16 + i + sv], acc);
    }
    // output 16 p + q of the tile sits at row p = (lane >> 4) + 4 g, column q = lane & 15
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int o = kProjWave * wave + 16 * (kk + 4 * g) + i;
      const int64_t t = tt + o;
      if (t >= t1) continue;
      const double pv = acc[g], rv = rP[pad16(512 + o)], ev = t < n ? (double)e[t] : 0.0;
      const double der = ev - rv, dpr = pv - rv, dep = ev - pv;
      en[0] += rv * rv;
      en[1] += der * der;
      en[2] += dpr * dpr;
      en[3] += pv * pv;
      en[4] += dep * dep;
      en[5] += ev * ev;
      if (P) P[(int64_t)b * ldp + t] = pv;
    }
  }
#pragma unroll
  for (int k = 0; k < kEnergies; ++k) {
    const double v = wave_sum(en[k]);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
  if (tid < kEnergies) ws.enp[((int64_t)b * ws.nso + s) * kEnergies + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

__global__ __launch_bounds__(64) void k_bss_final(const int* __restrict__ lens, int flen, BssWs ws, double* __restrict__ out) {
  __shared__ double en[kEnergies];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nsl = (int)(((int64_t)lens[b] + flen - 1 + kSlab - 1) / kSlab);
  if (tid < kEnergies) {
    const double* p = ws.enp + (int64_t)b * ws.nso * kEnergies + tid;
    double v = 0.0;
    for (int s = 0; s < nsl; ++s) v += p[(int64_t)s * kEnergies];
    en[tid] = v;
    ws.en[(int64_t)b * kEnergies + tid] = v;
  }
  __syncthreads();
  if (tid < 3) {
    // a silent target or a silent est (every sample exactly 0: a sum of squares of floats cannot underflow in double): NaN
    const double num = tid == 2 ? en[3] : en[0], den = tid == 0 ? en[1] : tid == 1 ? en[2] : en[4];
    double v;
    if (en[0] == 0.0 || en[5] == 0.0)
      v = NAN;
    else if (den == 0.0)
      v = INFINITY;
    else
      v = 10.0 * log10(num / den);
    out[(int64_t)b * 3 + tid] = v;
  }
}

namespace {

struct BssLayout {
  size_t lagp, ad, c, enp, en, end;
};
BssLayout bss_layout(int n, int ns, int nso) {
  auto up = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  BssLayout l{};
  size_t o = 0;
  l.lagp = o, o += up((size_t)n * ns * 2 * kF * sizeof(double));
  l.ad = o, o += up((size_t)n * 2 * kF * sizeof(double));
  l.c = o, o += up((size_t)n * kF * sizeof(double));
  l.enp = o, o += up((size_t)n * nso * kEnergies * sizeof(double));
  l.en = o, o += up((size_t)n * kEnergies * sizeof(double));
  l.end = o;
  return l;
}
inline int bss_slabs(int64_t len) { return (int)((len + kSlab - 1) / kSlab); }

}  // namespace

void bsseval_scores(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int flen, double* out,
                    const BssStageOut* stage, hipStream_t s) {
  VFX_CHECK(est && target && lengths && out && B > 0 && Lmax > 0,
            "vfx_bsseval: bad argument (NULL pointer, B = %d or Lmax = %d not positive)", B, Lmax);
  VFX_CHECK(flen >= 16 && flen <= kBssMaxFlen && flen % 16 == 0,
            "vfx_bsseval: a filter of %d taps is not supported (flen is a multiple of 16 in [16, %d])", flen, kBssMaxFlen);
  for (int b = 0; b < B; ++b)
    VFX_CHECK(lengths[b] >= 1 && lengths[b] <= Lmax, "vfx_bsseval: clip %d has %d samples (need 1 <= length <= Lmax = %d)", b, lengths[b],
              Lmax);
  // sub-batches of consecutive clips, each as many as keep its workspace under the cap (the whole batch for a stage copy)
  struct Sub { int b0, n, ns, nso; };
  std::vector<Sub> subs;
  size_t need = 0;
  for (int b0 = 0; b0 < B;) {
    Sub sb{b0, 0, 1, 1};
    while (b0 + sb.n < B && sb.n < kMaxVarlenClips) {
      const int ns = std::max(sb.ns, bss_slabs(lengths[b0 + sb.n]));
      const int nso = std::max(sb.nso, bss_slabs((int64_t)lengths[b0 + sb.n] + flen - 1));
      if (sb.n > 0 && !stage && bss_layout(sb.n + 1, ns, nso).end > kScoreWorkspaceBytes) break;
      sb.ns = ns;
      sb.nso = nso;
      ++sb.n;
    }
    need = std::max(need, bss_layout(sb.n, sb.ns, sb.nso).end);
    subs.push_back(sb);
    b0 += sb.n;
  }
  const int64_t ldp = (int64_t)Lmax + flen - 1;
  if (stage) {
    VFX_CHECK(subs.size() == 1, "vfx_op_bsseval_stage: at most %d clips", kMaxVarlenClips);
    const int64_t want[4] = {(int64_t)B * 2 * flen, (int64_t)B * flen, (int64_t)B * 5, (int64_t)B * ldp};
    VFX_CHECK(stage->stage >= 0 && stage->stage <= 3, "vfx_op_bsseval_stage: stage %d (need 0 .. 3)", stage->stage);
    VFX_CHECK(stage->out && stage->out_n == want[stage->stage], "vfx_op_bsseval_stage: stage %d of this batch writes %lld doubles (given %lld)",
              stage->stage, (long long)want[stage->stage], (long long)stage->out_n);
  }
  char* const base = h->score_ws.ensure(h, need, 0);
  int* const d_l = h->lens_row(LENS_BSS_SAMPLES);
  for (const Sub& sb : subs) {
    const BssLayout l = bss_layout(sb.n, sb.ns, sb.nso);
    BssWs ws{};
    ws.lagp = reinterpret_cast<double*>(base + l.lagp);
    ws.ad = reinterpret_cast<double*>(base + l.ad);
    ws.c = reinterpret_cast<double*>(base + l.c);
    ws.enp = reinterpret_cast<double*>(base + l.enp);
    ws.en = reinterpret_cast<double*>(base + l.en);
    ws.ns = sb.ns;
    ws.nso = sb.nso;
    const float* e = est + (int64_t)sb.b0 * Lmax;
    const float* r = target + (int64_t)sb.b0 * Lmax;
    double* P = nullptr;
    if (stage && stage->stage == 3) {  // what lies past a clip's own n + flen - 1 stays zero
      P = stage->out;
      VFX_HIP(hipMemsetAsync(P, 0, (size_t)stage->out_n * sizeof(double), s));
    }
    launch_set_frames(d_l, lengths + sb.b0, sb.n, s);
    hipLaunchKernelGGL(k_bss_corr, dim3(sb.ns, sb.n), dim3(256), 0, s, e, r, (int64_t)Lmax, d_l, flen, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bss_lags, dim3(sb.n), dim3(256), 0, s, d_l, flen, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bss_solve, dim3(sb.n), dim3(256), 0, s, flen, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bss_project, dim3(sb.nso, sb.n), dim3(256), 0, s, e, r, (int64_t)Lmax, d_l, flen, ws, P, ldp);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_bss_final, dim3(sb.n), dim3(64), 0, s, d_l, flen, ws, out + (int64_t)sb.b0 * 3);
    VFX_HIP(hipGetLastError());
    if (stage) {
      auto rows = [&](const double* src, int src_row, int row, int nrows) {
        VFX_HIP(hipMemcpy2DAsync(stage->out, (size_t)row * sizeof(double), src, (size_t)src_row * sizeof(double), (size_t)row * sizeof(double),
                                 (size_t)nrows, hipMemcpyDeviceToDevice, s));
      };
      if (stage->stage == 0) rows(ws.ad, kF, flen, 2 * B);
      if (stage->stage == 1) rows(ws.c, kF, flen, B);
      if (stage->stage == 2) rows(ws.en, kEnergies, 5, B);
      VFX_HIP(hipStreamSynchronize(s));
    }
  }
}

}  // namespace vfx
