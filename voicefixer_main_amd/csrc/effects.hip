// effects.hip -- the two array effects of MagicalEffects.effect that act on the samples themselves, for padded batches of float32 or
// float64 clips: quantification (dataloaders/augmentation/magical_effects.py:178-187) and time_dropout with its two smooth() patches
// (:169-176, tools/others/audio_op.py:152-174); both mirrored in simulate.py.
//
// Quantiser, per clip (level = 2 ** bins, L_j = -1 + (2 j + 1) / level for j < level -- exact doubles, the step is 2 / level):
//   1. p = max |x| over the clip's own samples, in the clip's dtype (a NaN sample makes it NaN, as np.max does)
//   2. s = x / p                         one correctly rounded division in the clip's dtype
//   3. k = #{j : L_j < (double)s}        np.digitize(s, L, right=True); a NaN s sorts above every level: k = level
//   4. idx = k - 1, and -1 -> level - 1  NumPy's index -1 is the LAST level: the negative peak comes out as +(1 - 1 / level) p
//   5. y = L_idx * (double)p             one double multiplication; the output is float64
// k is settled by a binary search that COMPARES s with the exact levels: no expression of s is ever rounded to an index (for a
// float64 clip s + 1 can round onto a level that s itself lies beside).  An arithmetic guess corrected against its neighbours was
// measured too and is no faster: the map pass is bound by its float64 stores.  Zero, infinite and NaN peaks take the same five steps.
//   k_fx_peaks     reads x            -> p (atomicMax on the bit pattern of |x|, 32 or 64 bits)
//   k_fx_quantize  reads x, writes y  -> rows zero from the clip's length up to ldy
//
// Time drop-out, per clip (start <= end, the reference's int(length * start) and int(length * start + length * trunk_length)):
//   k_fx_drop_copy    y = x with y[start : min(end, n)] = 0, rows zero from the clip's length up to ldy
//   k_fx_drop_smooth  one workgroup per clip; for c in (start, end), in that order, when c >= 50 and n - c >= 50: the 25 knots
//                     y[c - 50 + 4 i] are read AFTER everything before them was written (the second patch may overlap the first and
//                     the zeroed range), then y[c - 50 + t] = round(sum_i M[t][i] knot_i) for t < 96, the sum in double in ascending
//                     i, rounded once to the clip's dtype.  M (96, 25) is smooth()'s cubic interpolation as a matrix: the
//                     not-a-knot spline through 25 equidistant knots is linear in the knots (simulate.smooth_matrix builds it).
//
// The element-wise passes (k_fx_peaks, k_fx_quantize, k_fx_drop_copy) are grids over the batch in clip_batch.h's sample groups: a
// clip's result depends on the clip alone.
#include "clip_batch.h"
#include "vfx_internal.h"

#pragma clang fp contract(off)

namespace vfx {

constexpr int kFxThreads = 256;

struct QuantArgs {
  const void* x;             // (clips, ldx) float32 or float64
  double* y;                 // (clips, ldy)
  unsigned long long* bits;  // (clips) bit pattern of max |x| (the low 32 bits for float32), zeroed before the launches
  void* peaks;               // (clips) in x's dtype, or NULL
  int64_t ldx, ldy;
  int len[kFxMaxClips], bins[kFxMaxClips];
};

struct DropArgs {
  const void* x;         // (clips, ldx) float32 or float64
  void* y;               // (clips, ldy) x's dtype
  const double* smooth;  // (kFxSmoothRows, kFxSmoothKnots)
  int64_t ldx, ldy;
  int len[kFxMaxClips], start[kFxMaxClips], end[kFxMaxClips];  // start <= end <= len (the host clamps: a centre past the clip is skipped)
};

template <typename T>
__global__ __launch_bounds__(kFxThreads) void k_fx_peaks(const QuantArgs a) {
  using F = ClipType<T>;
  using Bits = typename F::Bits;
  constexpr int G = 16 / sizeof(T), K = kClipChunk / (G * kFxThreads);
  static_assert(kClipChunk == G * kFxThreads * K, "a chunk is whole groups of every thread");
  const int b = blockIdx.y;
  const int64_t n = a.len[b], c0 = (int64_t)blockIdx.x * kClipChunk;
  if (c0 >= n) return;
  const T* row = static_cast<const T*>(a.x) + (int64_t)b * a.ldx;
  const bool vec = clip_aligned(row);
  T v[K][G];
#pragma unroll
  for (int k = 0; k < K; ++k) clip_load(row, vec, c0 + G * (threadIdx.x + kFxThreads * k), n, v[k]);
  Bits peak = 0;  // (a sample past n was loaded as +0: bit pattern 0)
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < G; ++e) peak = max(peak, F::abs_bits(v[k][e]));
  __shared__ Bits wave_peak[kFxThreads / 64];
  clip_commit_peak<kFxThreads>(peak, reinterpret_cast<Bits*>(a.bits + b), wave_peak);
}

__device__ __forceinline__ double fx_level(int j, double inv_level) { return -1.0 + (double)(2 * j + 1) * inv_level; }  // exact

// steps 2-5 for one sample
template <typename T>
__device__ __forceinline__ double fx_quantize(T x, T p, double pd, int level, double inv_level) {
  const double s = (double)(x / p);
  int k = 0, hi = level;  // L_j < s for every j < k, and for no j >= hi
  if (s != s) k = level;  // a NaN s sorts above every level
  while (k < hi) {
    const int mid = (k + hi) >> 1;
    if (fx_level(mid, inv_level) < s)
      k = mid + 1;
    else
      hi = mid;
  }
  const int idx = k == 0 ? level - 1 : k - 1;
  return fx_level(idx, inv_level) * pd;
}

template <typename T>
__global__ __launch_bounds__(kFxThreads) void k_fx_quantize(const QuantArgs a) {
  using F = ClipType<T>;
  constexpr int G = 16 / sizeof(T), K = kClipChunk / (G * kFxThreads);
  const int b = blockIdx.y;
  const int64_t n = a.len[b], c0 = (int64_t)blockIdx.x * kClipChunk;
  if (c0 >= a.ldy) return;
  const T p = F::from_bits(*reinterpret_cast<const typename F::Bits*>(a.bits + b));
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.peaks) static_cast<T*>(a.peaks)[b] = p;
  const int level = 1 << a.bins[b];
  const double inv_level = 1.0 / (double)level, pd = (double)p;
  const T* row = static_cast<const T*>(a.x) + (int64_t)b * a.ldx;
  double* out = a.y + (int64_t)b * a.ldy;
  const bool vin = clip_aligned(row), vout = clip_aligned(out);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int64_t j = c0 + G * (threadIdx.x + kFxThreads * k);
    if (j >= a.ldy) break;
    double y[G];
#pragma unroll
    for (int e = 0; e < G; ++e) y[e] = 0.0;
    if (j < n) {
      T v[G];
      clip_load(row, vin, j, n, v);
#pragma unroll
      for (int e = 0; e < G; ++e)
        if (j + e < n) y[e] = fx_quantize(v[e], p, pd, level, inv_level);
    }
    clip_store(out, vout, j, a.ldy, y);
  }
}

template <typename T>
__global__ __launch_bounds__(kFxThreads) void k_fx_drop_copy(const DropArgs a) {
  constexpr int G = 16 / sizeof(T), K = kClipChunk / (G * kFxThreads);
  const int b = blockIdx.y;
  const int64_t n = a.len[b], c0 = (int64_t)blockIdx.x * kClipChunk, start = a.start[b], end = a.end[b];
  if (c0 >= a.ldy) return;
  const T* row = static_cast<const T*>(a.x) + (int64_t)b * a.ldx;
  T* out = static_cast<T*>(a.y) + (int64_t)b * a.ldy;
  const bool vin = clip_aligned(row), vout = clip_aligned(out);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int64_t j = c0 + G * (threadIdx.x + kFxThreads * k);
    if (j >= a.ldy) break;
    T y[G];
#pragma unroll
    for (int e = 0; e < G; ++e) y[e] = T(0);
    if (j < n) {
      T v[G];
      clip_load(row, vin, j, n, v);
#pragma unroll
      for (int e = 0; e < G; ++e)
        if (j + e < n && !(j + e >= start && j + e < end)) y[e] = v[e];
    }
    clip_store(out, vout, j, a.ldy, y);
  }
}

// one workgroup per clip, behind k_fx_drop_copy: the patch around `start`, then the one around `end`
template <typename T>
__global__ __launch_bounds__(128) void k_fx_drop_smooth(const DropArgs a) {
  __shared__ double knots[kFxSmoothKnots];
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t n = a.len[b];
  T* row = static_cast<T*>(a.y) + (int64_t)b * a.ldy;
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t c = pass ? a.end[b] : a.start[b];
    if (c < kFxSmoothHalf || n - c < kFxSmoothHalf) continue;  // (the same for every thread of the workgroup)
    T* patch = row + (c - kFxSmoothHalf);                       // knots up to patch[96] <= row[n - 4], writes up to patch[95]
    if (t < kFxSmoothKnots) knots[t] = (double)patch[kFxSmoothStep * t];
    __syncthreads();
    if (t < kFxSmoothRows) {
      const double* m = a.smooth + t * kFxSmoothKnots;
      double acc = m[0] * knots[0];
#pragma unroll
      for (int i = 1; i < kFxSmoothKnots; ++i) acc += m[i] * knots[i];
      patch[t] = (T)acc;
    }
    __syncthreads();  // the next patch reads what this one wrote
  }
}

template <typename T>
static void quantize_launches(const QuantArgs& a, int nb, int64_t nmax, hipStream_t s) {
  const dim3 block(kFxThreads);
  const dim3 pgrid((unsigned)((nmax + kClipChunk - 1) / kClipChunk), (unsigned)nb), qgrid((unsigned)((a.ldy + kClipChunk - 1) / kClipChunk), (unsigned)nb);
  hipLaunchKernelGGL(k_fx_peaks<T>, pgrid, block, 0, s, a);
  VFX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_fx_quantize<T>, qgrid, block, 0, s, a);
  VFX_HIP(hipGetLastError());
}

void launch_quantize(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* bins, double* y, int64_t ldy,
                     void* peaks, unsigned long long* bits, hipStream_t s) {
  const size_t esz = x_f64 ? sizeof(double) : sizeof(float);
  VFX_HIP(hipMemsetAsync(bits, 0, (size_t)B * sizeof(unsigned long long), s));
  QuantArgs a{};
  a.ldx = ldx;
  a.ldy = ldy;
  for_clip_slices<kFxMaxClips>(B, [&](int b0, int nb) {
    const int64_t nmax = narrow_clip_lengths(lengths, b0, nb, a.len);
    std::copy(bins + b0, bins + b0 + nb, a.bins);
    a.x = slice_rows(x, b0, ldx, esz);
    a.y = slice_rows(y, b0, ldy);
    a.bits = bits + b0;
    a.peaks = slice_rows(peaks, b0, 1, esz);
    if (x_f64)
      quantize_launches<double>(a, nb, nmax, s);
    else
      quantize_launches<float>(a, nb, nmax, s);
  });
}

template <typename T>
static void drop_launches(const DropArgs& a, int nb, hipStream_t s) {
  const dim3 grid((unsigned)((a.ldy + kClipChunk - 1) / kClipChunk), (unsigned)nb);
  hipLaunchKernelGGL(k_fx_drop_copy<T>, grid, dim3(kFxThreads), 0, s, a);
  VFX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_fx_drop_smooth<T>, dim3((unsigned)nb), dim3(128), 0, s, a);
  VFX_HIP(hipGetLastError());
}

void launch_time_dropout(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int64_t* starts, const int64_t* ends,
                         const double* smooth, void* y, int64_t ldy, hipStream_t s) {
  const size_t esz = x_f64 ? sizeof(double) : sizeof(float);
  DropArgs a{};
  a.smooth = smooth;
  a.ldx = ldx;
  a.ldy = ldy;
  for_clip_slices<kFxMaxClips>(B, [&](int b0, int nb) {
    narrow_clip_lengths(lengths, b0, nb, a.len);
    for (int i = 0; i < nb; ++i) {
      // an index past the clip zeroes nothing and is no centre of a patch (n - c < 50), and so is the clip's length
      a.start[i] = (int)std::min(starts[b0 + i], lengths[b0 + i]);
      a.end[i] = (int)std::min(ends[b0 + i], lengths[b0 + i]);
    }
    a.x = slice_rows(x, b0, ldx, esz);
    a.y = slice_rows(y, b0, ldy, esz);
    if (x_f64)
      drop_launches<double>(a, nb, s);
    else
      drop_launches<float>(a, nb, s);
  });
}

}  // namespace vfx
