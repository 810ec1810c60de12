// stoi.hip -- STOI, the short-time objective intelligibility measure (Taal, Hendriks, Heusdens, Jensen, IEEE TASLP 2011; restated from
// the paper, the authors' MATLAB and pystoi's stoi(extended=False)), per clip of a padded batch, gfx950.  Float32 clips in, float64
// from the first multiply on.  `target` is the clean signal (pystoi's x), `est` the processed one (y).
//
//   k_stoi_resample     resample_poly(x, up, down, window=taps) to 10 kHz: y[o] = sum_k x[k] taps[hl + o down - k up], k descending, one
//                       thread per output (4 outputs per thread).  The filter is walked in steps of `up` taps: the phases of T steps
//                       (T up <= 4096 taps) are staged in LDS at a time, never the whole table.  Without taps (up == down): a widening copy
//   k_stoi_frame_energy one wave per (clip, frame): 20 log10(|w . target frame| + EPS); frames start at range(0, n - 256, 128)
//   k_stoi_mask         one workgroup per clip: the maximum, the keep mask (max - 40 - e < 0), its exclusive scan (kept index ->
//                       source frame) and the count
//   k_stoi_bands        one workgroup per (clip, STFT frame m < kept - 1): the 256 samples of the overlap-added kept frames are
//                       rebuilt from the (at most three) kept source frames that cover them, windowed again, and bins 7..218 of the
//                       512-point DFT taken directly from an LDS twiddle table (one bin per thread, both signals); then the 15
//                       third-octave band powers and their square roots
//   k_stoi_score        per (clip, segment of 30 frames, band): normalise, clip at -15 dB SDR, correlate; the 15 terms of a segment
//                       summed in band order
//   k_stoi_final        one workgroup per clip: its segments summed in a fixed order -> d, or 1e-5 with fewer than 30 STFT frames
//
// Frame-count convention: range(0, n - 256, 128) for both the silent-frame removal and the STFT (the authors' MATLAB 1:hop:(n - N);
// the last aligned frame is NOT taken).  Everything is cut from the clip's own extent: nothing at or past a clip's length, frames
// or segments is read, so a clip's score does not depend on the batch it is in.  No float atomics.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "vfx_internal.h"

namespace vfx {

namespace {

constexpr int kWaves = 4;
constexpr int kTapLds = 4096;             // taps staged per step of k_stoi_resample (T = kTapLds / up whole tap steps)
constexpr int kResampleOutPerThread = 4;  // outputs per thread: a workgroup writes 1024 consecutive outputs
constexpr int kResampleTile = 256 * kResampleOutPerThread;
constexpr int kBin0 = 7, kBins = 212;     // rFFT bins 7..218: the union of the 15 bands
constexpr int kSegsPerBlock = 16;         // k_stoi_score: 16 lanes (15 bands) per segment
static_assert(kStoiMaxUp * 4 <= kTapLds, "at least four tap steps per staging");
static_assert(kStoiFrame == 256 && kStoiHop == 128, "one sample per thread, two hops per frame");

// the workspace of one sub-batch: n clips of at most N samples at 10 kHz and Fm frames
struct StoiWs {
  double* rs;    // [n][2][N]       est, target at 10 kHz
  double* en;    // [n][Fm]         frame energies of the target, dB
  int* mask;     // [n][Fm]         1 = kept
  int* map;      // [n][Fm]         kept index -> source frame
  int* cnt;      // [n]             kept frames
  double* pw;    // [n][2][Fm][15]  band powers (null unless asked for), STFT frames m < cnt - 1
  double* tob;   // [n][2][Fm][15]  their square roots
  double* seg;   // [n][Fm]         per-segment sums of the 15 band correlations
  int64_t N;
  int Fm;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// np.hanning(258)[1:-1][n]
__device__ __forceinline__ double stoi_window(int n) { return 0.5 + 0.5 * cospi((double)(2 * n - 255) / 257.0); }

}  // namespace

__global__ __launch_bounds__(256) void k_stoi_resample(const float* __restrict__ est, const float* __restrict__ tgt, int64_t ld,
                                                       const int* __restrict__ lens, int up, int down, const double* __restrict__ taps,
                                                       int ntaps, StoiWs ws) {
  __shared__ double ht[kTapLds];
  const int b = blockIdx.y >> 1, sig = blockIdx.y & 1, tid = threadIdx.x;
  const int64_t n = lens[b];
  const int64_t nout = stoi_out_len(n, up, down);
  const int64_t o0 = (int64_t)blockIdx.x * kResampleTile;
  if (o0 >= nout) return;
  const float* x = (sig ? tgt : est) + (int64_t)b * ld;
  double* y = ws.rs + ((int64_t)b * 2 + sig) * ws.N;
  if (ntaps == 0) {  // already at 10 kHz
#pragma unroll
    for (int r = 0; r < kResampleOutPerThread; ++r) {
      const int64_t o = o0 + tid + 256 * r;
      if (o < nout) y[o] = (double)x[o];
    }
    return;
  }
  const int hl = (ntaps - 1) / 2;
  int phi[kResampleOutPerThread];
  int64_t kmax[kResampleOutPerThread];
  double acc[kResampleOutPerThread];
#pragma unroll
  for (int r = 0; r < kResampleOutPerThread; ++r) {
    const int64_t a = hl + (o0 + tid + 256 * r) * down;
    phi[r] = (int)(a % up);
    kmax[r] = a / up;
    acc[r] = 0.0;
  }
  const int T = kTapLds / up;
  const int steps = (ntaps + up - 1) / up;
  for (int t0 = 0; t0 < steps; t0 += T) {
    __syncthreads();
    const int64_t j0 = (int64_t)t0 * up;
    for (int i = tid; i < T * up; i += 256) ht[i] = j0 + i < ntaps ? taps[j0 + i] : 0.0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kResampleOutPerThread; ++r) {
      if (o0 + tid + 256 * r >= nout) continue;
      int64_t k = kmax[r] - t0;
      int j = phi[r];
      for (int t = 0; t < T && k >= 0; ++t, --k, j += up)
        if (k < n) acc[r] += (double)x[k] * ht[j];
    }
  }
#pragma unroll
  for (int r = 0; r < kResampleOutPerThread; ++r) {
    const int64_t o = o0 + tid + 256 * r;
    if (o < nout) y[o] = acc[r];
  }
}

__global__ __launch_bounds__(256) void k_stoi_frame_energy(const int* __restrict__ frames, StoiWs ws) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= frames[b]) return;
  const double* x = ws.rs + ((int64_t)b * 2 + 1) * ws.N + (int64_t)i * kStoiHop;
  double v = 0.0;
#pragma unroll
  for (int r = 0; r < kStoiFrame / 64; ++r) {
    const int n = lane + 64 * r;
    const double f = stoi_window(n) * x[n];
    v += f * f;
  }
  v = wave_sum(v);
  if (lane == 0) ws.en[(int64_t)b * ws.Fm + i] = 20.0 * log10(sqrt(v) + DBL_EPSILON);
}

__global__ __launch_bounds__(256) void k_stoi_mask(const int* __restrict__ frames, StoiWs ws) {
  __shared__ double mx[256];
  __shared__ int kept[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nf = frames[b];
  const double* en = ws.en + (int64_t)b * ws.Fm;
  double m = -INFINITY;
  for (int i = tid; i < nf; i += 256) m = fmax(m, en[i]);
  mx[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) mx[tid] = fmax(mx[tid], mx[tid + o]);
    __syncthreads();
  }
  m = mx[0];
  // a contiguous run of frames per thread: its kept count, then the counts of the threads before it
  const int per = (nf + 255) / 256;
  const int i0 = min(nf, tid * per), i1 = min(nf, i0 + per);
  int c = 0;
  for (int i = i0; i < i1; ++i) c += (m - 40.0 - en[i] < 0.0) ? 1 : 0;
  kept[tid] = c;
  __syncthreads();
  int at = 0;
  for (int t = 0; t < tid; ++t) at += kept[t];
  int* mask = ws.mask + (int64_t)b * ws.Fm;
  int* map = ws.map + (int64_t)b * ws.Fm;
  for (int i = i0; i < i1; ++i) {
    const int k = (m - 40.0 - en[i] < 0.0) ? 1 : 0;
    mask[i] = k;
    if (k) map[at++] = i;
  }
  if (tid == 255) ws.cnt[b] = at;
}

__global__ __launch_bounds__(256) void k_stoi_bands(StoiWs ws) {
  __shared__ double wl[kStoiFrame], cs[512], sn[512], xs[2][kStoiFrame], pl[2][kBins];
  const int b = blockIdx.y, m = blockIdx.x, tid = threadIdx.x;
  const int kept = ws.cnt[b];
  if (m >= kept - 1) return;
  wl[tid] = stoi_window(tid);
  for (int i = tid; i < 512; i += 256) {
    cs[i] = cospi((double)i / 256.0);
    sn[i] = sinpi((double)i / 256.0);
  }
  __syncthreads();
  // sample 128 m + tid of the overlap-added signal lies in hop block q: kept frame q - 1 (its second half) + kept frame q (its first)
  const int* map = ws.map + (int64_t)b * ws.Fm;
  const int q = m + (tid >> 7), off = tid & 127;  // q <= kept - 1
#pragma unroll
  for (int sig = 0; sig < 2; ++sig) {
    const double* x = ws.rs + ((int64_t)b * 2 + sig) * ws.N;
    double v = 0.0;
    if (q >= 1) v = wl[kStoiHop + off] * x[(int64_t)map[q - 1] * kStoiHop + kStoiHop + off];
    v += wl[off] * x[(int64_t)map[q] * kStoiHop + off];
    xs[sig][tid] = wl[tid] * v;
  }
  __syncthreads();
  if (tid < kBins) {
    const int k = kBin0 + tid;
    double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
    int idx = 0;
    for (int n = 0; n < kStoiFrame; ++n) {
      const double c = cs[idx], s = sn[idx], e = xs[0][n], g = xs[1][n];
      re0 += e * c;
      im0 += e * s;
      re1 += g * c;
      im1 += g * s;
      idx = (idx + k) & 511;
    }
    pl[0][tid] = re0 * re0 + im0 * im0;
    pl[1][tid] = re1 * re1 + im1 * im1;
  }
  __syncthreads();
  if (tid < 2 * kStoiBands) {
    // the rFFT bins nearest to 150 * 2^((2 j -+ 1) / 6) Hz on linspace(0, 10000, 513), half-open
    static constexpr int edge[kStoiBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
    const int sig = tid / kStoiBands, j = tid % kStoiBands;
    double p = 0.0;
    for (int k = edge[j]; k < edge[j + 1]; ++k) p += pl[sig][k - kBin0];
    const int64_t o = (((int64_t)b * 2 + sig) * ws.Fm + m) * kStoiBands + j;
    if (ws.pw) ws.pw[o] = p;
    ws.tob[o] = sqrt(p);
  }
}

__global__ __launch_bounds__(256) void k_stoi_score(StoiWs ws) {
  __shared__ double term[kSegsPerBlock][16];
  const int b = blockIdx.y, g = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int nseg = ws.cnt[b] - 1 - (kStoiSegment - 1);  // STFT frames - 29
  if ((int)blockIdx.x * kSegsPerBlock >= nseg) return;
  const int sidx = blockIdx.x * kSegsPerBlock + g;      // the 30 columns [sidx, sidx + 30)
  const bool on = sidx < nseg && j < kStoiBands;
  double d = 0.0;
  if (on) {
    const double* y = ws.tob + (((int64_t)b * 2 + 0) * ws.Fm + sidx) * kStoiBands + j;
    const double* x = ws.tob + (((int64_t)b * 2 + 1) * ws.Fm + sidx) * kStoiBands + j;
    double xx = 0.0, yy = 0.0;
    for (int f = 0; f < kStoiSegment; ++f) {
      const double xv = x[f * kStoiBands], yv = y[f * kStoiBands];
      xx += xv * xv;
      yy += yv * yv;
    }
    const double alpha = sqrt(xx) / (sqrt(yy) + DBL_EPSILON);
    const double bound = 1.0 + 5.623413251903491;  // 1 + 10^(15 / 20): beta = -15 dB
    double sx = 0.0, sy = 0.0;
    for (int f = 0; f < kStoiSegment; ++f) {
      const double xv = x[f * kStoiBands];
      sx += xv;
      sy += fmin(alpha * y[f * kStoiBands], xv * bound);
    }
    const double mx = sx / kStoiSegment, my = sy / kStoiSegment;
    double cxx = 0.0, cyy = 0.0, cxy = 0.0;
    for (int f = 0; f < kStoiSegment; ++f) {
      const double xv = x[f * kStoiBands];
      const double xc = xv - mx, yc = fmin(alpha * y[f * kStoiBands], xv * bound) - my;
      cxx += xc * xc;
      cyy += yc * yc;
      cxy += xc * yc;
    }
    d = cxy / ((sqrt(cxx) + DBL_EPSILON) * (sqrt(cyy) + DBL_EPSILON));
  }
  term[g][j] = d;
  __syncthreads();
  if (on && j == 0) {
    double s = 0.0;
    for (int k = 0; k < kStoiBands; ++k) s += term[g][k];
    ws.seg[(int64_t)b * ws.Fm + sidx] = s;
  }
}

__global__ __launch_bounds__(256) void k_stoi_final(StoiWs ws, double* __restrict__ out) {
  __shared__ double red[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nseg = ws.cnt[b] - 1 - (kStoiSegment - 1);
  if (nseg < 1) {  // fewer than 30 STFT frames: pystoi's warning value
    if (tid == 0) out[b] = 1e-5;
    return;
  }
  double v = 0.0;
  for (int i = tid; i < nseg; i += 256) v += ws.seg[(int64_t)b * ws.Fm + i];
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) out[b] = (((red[0] + red[1]) + red[2]) + red[3]) / ((double)nseg * kStoiBands);
}

namespace {

struct StoiLayout {
  size_t rs, en, mask, map, cnt, pw, tob, seg, end;
};
StoiLayout stoi_layout(int n, int64_t N, int Fm, bool powers) {
  auto up = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  StoiLayout l{};
  const size_t bands = (size_t)n * 2 * Fm * kStoiBands * sizeof(double);
  size_t o = 0;
  l.rs = o, o += up((size_t)n * 2 * N * sizeof(double));
  l.en = o, o += up((size_t)n * Fm * sizeof(double));
  l.mask = o, o += up((size_t)n * Fm * sizeof(int));
  l.map = o, o += up((size_t)n * Fm * sizeof(int));
  l.cnt = o, o += up((size_t)n * sizeof(int));
  l.pw = o, o += powers ? up(bands) : 0;
  l.tob = o, o += up(bands);
  l.seg = o, o += up((size_t)n * Fm * sizeof(double));
  l.end = o;
  return l;
}

}  // namespace

void stoi_scores(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int up, int down,
                 const double* taps, int ntaps, double* out, const StoiStageOut* stage, hipStream_t s) {
  VFX_CHECK(est && target && lengths && out && B > 0 && Lmax > 0, "vfx_stoi: bad argument (NULL pointer, B = %d or Lmax = %d not positive)",
            B, Lmax);
  VFX_CHECK(up > 0 && down > 0, "vfx_stoi: bad rates %d/%d", up, down);
  const int g = std::gcd(up, down);
  up /= g;
  down /= g;
  if (up == down) {
    ntaps = 0;
  } else {
    VFX_CHECK(up <= kStoiMaxUp && down <= kStoiMaxDown,
              "vfx_stoi: the rate ratio %d/%d is not supported (the resampler takes a reduced up <= %d and down <= %d)", up, down, kStoiMaxUp,
              kStoiMaxDown);
    VFX_CHECK(ntaps >= 1 && ntaps <= kStoiMaxTaps && (ntaps & 1),
              "vfx_stoi: a filter of %d taps is not supported (the resampler takes an odd count <= %d)", ntaps, kStoiMaxTaps);
    VFX_CHECK(taps != nullptr, "vfx_stoi: taps is NULL for %d/%d", up, down);
  }
  for (int b = 0; b < B; ++b)
    VFX_CHECK(lengths[b] >= 1 && lengths[b] <= Lmax, "vfx_stoi: clip %d has %d samples (need 1 <= length <= Lmax = %d)", b, lengths[b], Lmax);
  VFX_CHECK(stoi_out_len(Lmax, up, down) <= INT32_MAX, "vfx_stoi: Lmax = %d samples at %d/%d are more than 2^31 - 1 at 10 kHz", Lmax, up, down);
  std::vector<int> n10(B), frames(B);
  for (int b = 0; b < B; ++b) {
    n10[b] = (int)stoi_out_len(lengths[b], up, down);
    frames[b] = stoi_frames(n10[b]);
  }
  // sub-batches of consecutive clips, each as many as keep its workspace under the cap (the whole batch for a stage copy)
  struct Sub { int b0, n; int64_t N; int Fm; };
  std::vector<Sub> subs;
  const bool powers = stage && stage->stage == 2;
  size_t need = 0;
  for (int b0 = 0; b0 < B;) {
    Sub sb{b0, 0, 1, 1};
    while (b0 + sb.n < B && sb.n < kMaxVarlenClips) {
      const int64_t N = std::max<int64_t>(sb.N, n10[b0 + sb.n]);
      const int Fm = std::max(sb.Fm, frames[b0 + sb.n]);
      if (sb.n > 0 && !stage && stoi_layout(sb.n + 1, N, Fm, powers).end > kScoreWorkspaceBytes) break;
      sb.N = N;
      sb.Fm = Fm;
      ++sb.n;
    }
    need = std::max(need, stoi_layout(sb.n, sb.N, sb.Fm, powers).end);
    subs.push_back(sb);
    b0 += sb.n;
  }
  if (stage) {
    VFX_CHECK(subs.size() == 1, "vfx_op_stoi_stage: at most %d clips", kMaxVarlenClips);
    const Sub& sb = subs[0];
    const int64_t rows = (int64_t)B * 2, want[4] = {rows * sb.N, (int64_t)B * sb.Fm, rows * sb.Fm * kStoiBands, rows * sb.Fm * kStoiBands};
    const int64_t iwant[4] = {B, (int64_t)B * (1 + sb.Fm), B, B};
    VFX_CHECK(stage->stage >= 0 && stage->stage <= 3, "vfx_op_stoi_stage: stage %d (need 0 .. 3)", stage->stage);
    VFX_CHECK(stage->out && stage->iout && stage->out_n == want[stage->stage] && stage->iout_n == iwant[stage->stage],
              "vfx_op_stoi_stage: stage %d of this batch writes %lld doubles and %lld ints (given %lld and %lld)", stage->stage,
              (long long)want[stage->stage], (long long)iwant[stage->stage], (long long)stage->out_n, (long long)stage->iout_n);
  }
  char* const base = h->score_ws.ensure(h, need, 0);
  int* const d_l = h->lens_row(LENS_STOI_SAMPLES);
  int* const d_n = h->lens_row(LENS_STOI_OUT);
  int* const d_f = h->lens_row(LENS_STOI_FRAMES);
  for (const Sub& sb : subs) {
    const StoiLayout l = stoi_layout(sb.n, sb.N, sb.Fm, powers);
    if (stage) VFX_HIP(hipMemsetAsync(base, 0, l.end, s));  // what lies past a clip's own extent is copied out as zeros
    StoiWs ws{};
    ws.rs = reinterpret_cast<double*>(base + l.rs);
    ws.en = reinterpret_cast<double*>(base + l.en);
    ws.mask = reinterpret_cast<int*>(base + l.mask);
    ws.map = reinterpret_cast<int*>(base + l.map);
    ws.cnt = reinterpret_cast<int*>(base + l.cnt);
    ws.pw = powers ? reinterpret_cast<double*>(base + l.pw) : nullptr;
    ws.tob = reinterpret_cast<double*>(base + l.tob);
    ws.seg = reinterpret_cast<double*>(base + l.seg);
    ws.N = sb.N;
    ws.Fm = sb.Fm;
    launch_set_frames(d_l, lengths + sb.b0, sb.n, s);
    launch_set_frames(d_n, n10.data() + sb.b0, sb.n, s);
    launch_set_frames(d_f, frames.data() + sb.b0, sb.n, s);
    const unsigned tiles = (unsigned)((sb.N + kResampleTile - 1) / kResampleTile);
    hipLaunchKernelGGL(k_stoi_resample, dim3(tiles, 2 * sb.n), dim3(256), 0, s, est + (int64_t)sb.b0 * Lmax,
                       target + (int64_t)sb.b0 * Lmax, (int64_t)Lmax, d_l, up, down, taps, ntaps, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_stoi_frame_energy, dim3((sb.Fm + kWaves - 1) / kWaves, sb.n), dim3(256), 0, s, d_f, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_stoi_mask, dim3(sb.n), dim3(256), 0, s, d_f, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_stoi_bands, dim3(sb.Fm, sb.n), dim3(256), 0, s, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_stoi_score, dim3((sb.Fm + kSegsPerBlock - 1) / kSegsPerBlock, sb.n), dim3(256), 0, s, ws);
    VFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_stoi_final, dim3(sb.n), dim3(256), 0, s, ws, out + sb.b0);
    VFX_HIP(hipGetLastError());
    if (stage) {
      auto copy = [&](void* dst, const void* src, size_t bytes) { VFX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s)); };
      switch (stage->stage) {
        case 0:
          copy(stage->out, ws.rs, (size_t)stage->out_n * sizeof(double));
          copy(stage->iout, d_n, (size_t)B * sizeof(int));
          break;
        case 1:
          copy(stage->out, ws.en, (size_t)stage->out_n * sizeof(double));
          copy(stage->iout, ws.cnt, (size_t)B * sizeof(int));
          copy(stage->iout + B, ws.mask, (size_t)B * sb.Fm * sizeof(int));
          break;
        default:
          copy(stage->out, stage->stage == 2 ? ws.pw : ws.tob, (size_t)stage->out_n * sizeof(double));
          copy(stage->iout, ws.cnt, (size_t)B * sizeof(int));
      }
      VFX_HIP(hipStreamSynchronize(s));
    }
  }
}

}  // namespace vfx
