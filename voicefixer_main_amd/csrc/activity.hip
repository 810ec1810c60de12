// activity.hip -- the peak-threshold silence functions of the reference's data preparation (tools/others/audio_op.py:79-150:
// trim_tail_empty, trim_head_empty, trim_empty, has_long_empty, get_all_active_segment_index / is_valid_signal) for padded batches of
// float32 or float64 clips, gfx950.  Every one of them is decided by window peaks max |x[i]| over windows of ONE clip:
//
//   k_window_peaks     P[set][b][k] = max |x_b[o + k S + i]|, 0 <= i < W, k < count: one WAVE per window, in clip_batch.h's 16-byte
//                      sample groups at row-relative indices, the groups that straddle a window's ends masked sample by sample.  The
//                      maximum is taken over ClipType<T>::abs_bits patterns: order-independent, and a NaN lands above every finite
//                      value, as np.max gives NaN.  A launch holds one or two window grids of every clip (blockIdx.z: trim_empty needs
//                      the grid that ends at n and the grid that starts at 0).  In reflect mode an index j < 0 stands for x[-j] and
//                      j >= n for x[2 (n - 1) - j] (np.pad(..., mode="reflect")): a maximum over reflected indices is the maximum over
//                      the source ranges they fall on, so the window is up to three plain ranges of the clip.
//   k_activity_decide  one workgroup per clip: the bounds, the flag or the labels from the clip's peaks BY INDEX (the last active
//                      window of the tail grid is a max over k, the first of the head grid a min, the flag an or) -- no walk.  The
//                      threshold arrives rounded to the clip's dtype and is compared there; a NaN peak is neither < nor > it.
//
// A window of 882 samples is 3.5 kB: four 16-byte loads per lane of a wave, no LDS and no barrier, where a 256-thread workgroup would
// leave 35 threads idle and pay a barrier for a 14 us kernel.  The 3-s windows of has_long_empty overlap by two thirds and are re-read;
// they are a handful per clip.  Nothing at or past a clip's length is read.
#include "clip_batch.h"
#include "vfx_internal.h"

namespace vfx {

namespace {

constexpr int kActThreads = 256, kActWaves = kActThreads / 64;

struct PeakArgs {
  const void* x;  // (clips, ldx) float32 or float64
  void* peaks;    // (sets, clips, ldp) bit patterns of x's dtype
  int64_t ldx, ldp, W, S;
  int reflect, nb;
  int len[kActMaxClips];
  int origin[2][kActMaxClips];  // of window 0, relative to the clip's first sample (negative: reflect mode's left pad)
  int count[2][kActMaxClips];   // windows of the clip in each grid
};

struct DecideArgs {
  const void* peaks;
  int64_t ldp, seg, ldf;
  double threshold;  // rounded to the clips' dtype by the host
  int mode, nb;
  int64_t *start, *stop, *counts;
  int* flag;
  uint8_t* labels;
  int len[kActMaxClips];
  int count[kActMaxClips];  // windows of grid 0 (the flag and the labels)
};

// max |row[i]| over lo <= i < hi of this lane's groups (0 <= lo, hi <= n); the wave's lanes take consecutive groups
template <typename T>
__device__ __forceinline__ typename ClipType<T>::Bits range_peak(const T* row, bool vec, int64_t lo, int64_t hi, int64_t n, int lane) {
  using F = ClipType<T>;
  constexpr int G = 16 / sizeof(T);
  typename F::Bits peak = 0;
  if (lo >= hi) return peak;
#pragma unroll 4
  for (int64_t j = lo / G * G + G * lane; j < hi; j += 64 * G) {
    T v[G];
    clip_load(row, vec, j, n, v);
#pragma unroll
    for (int e = 0; e < G; ++e)
      if (j + e >= lo && j + e < hi) peak = max(peak, F::abs_bits(v[e]));
  }
  return peak;
}

template <typename T>
__global__ __launch_bounds__(kActThreads) void k_window_peaks(const PeakArgs a) {
  using Bits = typename ClipType<T>::Bits;
  const int b = blockIdx.y, set = blockIdx.z, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * kActWaves + (threadIdx.x >> 6);
  if (k >= a.count[set][b]) return;  // (the whole wave: no barrier follows)
  const int64_t n = a.len[b];
  const T* row = static_cast<const T*>(a.x) + (int64_t)b * a.ldx;
  const bool vec = clip_aligned(row);
  const int64_t s = a.origin[set][b] + k * a.S, e = s + a.W;
  Bits peak = range_peak(row, vec, max(s, (int64_t)0), min(e, n), n, lane);
  if (a.reflect) {
    // j in [s, min(e, 0)) reads x[-j]: the indices [max(1 - e, 1), 1 - s); j in [max(s, n), e) reads x[2 (n - 1) - j]: the indices
    // [2 n - 1 - e, 2 n - 1 - max(s, n)).  The host has checked n > pad, which keeps both inside the clip; the clamps cost nothing.
    if (s < 0) peak = max(peak, range_peak(row, vec, max(1 - e, (int64_t)1), min(1 - s, n), n, lane));
    if (e > n) peak = max(peak, range_peak(row, vec, max(2 * n - 1 - e, (int64_t)0), min(2 * n - 1 - max(s, n), n), n, lane));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) peak = max(peak, (Bits)__shfl_xor(peak, d));
  if (lane == 0) static_cast<Bits*>(a.peaks)[((int64_t)set * a.nb + b) * a.ldp + k] = peak;
}

template <typename T>
__global__ __launch_bounds__(kActThreads) void k_activity_decide(const DecideArgs a) {
  using F = ClipType<T>;
  using Bits = typename F::Bits;
  __shared__ int last_active, first_active, any_quiet;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t n = a.len[b];
  const T thr = (T)a.threshold;
  const Bits* const p0 = static_cast<const Bits*>(a.peaks) + (int64_t)b * a.ldp;
  if (a.mode == ACT_FRAMES) {  // is_valid_signal: peak > threshold, strictly
    const int count = a.count[b];
    uint8_t* out = a.labels + (int64_t)b * a.ldf;
    for (int64_t k = tid; k < a.ldf; k += kActThreads) out[k] = k < count && F::from_bits(p0[k]) > thr ? 1 : 0;
    if (tid == 0 && a.counts) a.counts[b] = count;
    return;
  }
  if (tid == 0) {
    last_active = -1;
    first_active = 0x7fffffff;
    any_quiet = 0;
  }
  __syncthreads();
  if (a.mode == ACT_LONG) {  // any window with peak < threshold
    const int count = a.count[b];
    int quiet = 0;
    for (int k = tid; k < count; k += kActThreads) quiet |= F::from_bits(p0[k]) < thr ? 1 : 0;
    if (quiet) atomicOr(&any_quiet, 1);
    __syncthreads();
    if (tid == 0) a.flag[b] = any_quiet;
    return;
  }
  // the trims.  Grid 0 of the peaks is the first grid the mode needs: the tail grid (origin n % seg) unless the mode is the head alone.
  const int64_t seg = a.seg, m = n / seg, r = n % seg;
  const Bits* const p_head = a.mode == ACT_BOTH ? p0 + (int64_t)a.nb * a.ldp : p0;
  int64_t start = 0, stop = n;
  bool none = false;  // (the same for every thread: what it rests on comes through LDS)
  if (a.mode != ACT_HEAD) {
    // the walk from the last window stops at the last window k that is not quiet, or at the window whose end is seg (k = 0 of a grid
    // with r = 0), which it never tests; L = the end of that window, r when there is none
    int last = -1;
    for (int k = tid; k < m; k += kActThreads)
      if (!(F::from_bits(p0[k]) < thr)) last = k;
    if (last >= 0) atomicMax(&last_active, last);
    __syncthreads();
    int64_t kk = last_active;
    if (r == 0 && kk < 0) kk = 0;
    const int64_t L = r + (kk + 1) * seg;
    if (n < seg || L < seg)
      none = true;
    else
      stop = L == n ? n : L - seg;  // (one further segment goes; L == seg leaves an empty clip)
  }
  if (a.mode != ACT_TAIL && !none) {
    // on the first `stop` samples: the walk from 0 stops at the first window that is not quiet, or at the first s = k seg that is
    // not < stop - seg
    const int64_t kq = stop > seg ? (stop - 1) / seg : 0;  // ceil((stop - seg) / seg): every window below it ends before `stop`
    int first = 0x7fffffff;
    for (int k = tid; k < kq; k += kActThreads)
      if (!(F::from_bits(p_head[k]) < thr)) {
        first = k;
        break;
      }
    if (first != 0x7fffffff) atomicMin(&first_active, first);
    __syncthreads();
    const int64_t s = min((int64_t)first_active, kq) * seg;
    if (s >= stop - seg)
      none = true;
    else
      start = s == 0 ? 0 : s - seg;  // (one quiet segment stays)
  }
  if (tid == 0) {
    a.start[b] = none ? -1 : start;
    a.stop[b] = none ? -1 : stop;
  }
}

template <typename T>
void activity_launches(const PeakArgs& p, const DecideArgs& d, int sets, int64_t most, hipStream_t s) {
  if (most > 0) {
    const dim3 grid((unsigned)((most + kActWaves - 1) / kActWaves), (unsigned)p.nb, (unsigned)sets);
    hipLaunchKernelGGL(k_window_peaks<T>, grid, dim3(kActThreads), 0, s, p);
    VFX_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_activity_decide<T>, dim3((unsigned)p.nb), dim3(kActThreads), 0, s, d);
  VFX_HIP(hipGetLastError());
}

}  // namespace

void launch_activity(int mode, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, int64_t W, int64_t S,
                     double threshold, void* ws, int64_t ldp, int64_t* start, int64_t* stop, int* flag, uint8_t* labels, int64_t ldf,
                     int64_t* counts, hipStream_t s) {
  const size_t esz = x_f64 ? sizeof(double) : sizeof(float);
  const int sets = mode == ACT_BOTH ? 2 : 1;
  PeakArgs p{};
  DecideArgs d{};
  p.peaks = ws;
  d.peaks = ws;
  p.ldx = ldx;
  p.ldp = d.ldp = ldp;
  p.W = W;
  p.S = S;
  p.reflect = mode == ACT_FRAMES;
  d.seg = W;
  d.ldf = ldf;
  d.threshold = threshold;
  d.mode = mode;
  for_clip_slices<kActMaxClips>(B, [&](int b0, int nb) {
    narrow_clip_lengths(lengths, b0, nb, p.len);
    narrow_clip_lengths(lengths, b0, nb, d.len);
    int64_t most = 0;
    for (int i = 0; i < nb; ++i) {
      const int64_t n = lengths[b0 + i], c = activity_windows(mode, n, W, S);
      for (int g = 0; g < sets; ++g) p.count[g][i] = (int)c;
      d.count[i] = (int)c;
      p.origin[0][i] = (int)activity_origin(mode, n, W, S);
      p.origin[1][i] = 0;  // the head grid behind the tail grid
      most = std::max(most, c);
    }
    p.nb = d.nb = nb;
    p.x = slice_rows(x, b0, ldx, esz);
    d.start = slice_rows(start, b0, 1);
    d.stop = slice_rows(stop, b0, 1);
    d.flag = slice_rows(flag, b0, 1);
    d.labels = slice_rows(labels, b0, ldf);
    d.counts = slice_rows(counts, b0, 1);
    if (x_f64)
      activity_launches<double>(p, d, sets, most, s);
    else
      activity_launches<float>(p, d, sets, most, s);
  });
}

}  // namespace vfx
