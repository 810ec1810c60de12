// clip_batch.h -- what the waveform kernels for padded batches of clips share (resample, sosfilt, reverb, mix, effects): x (clips, ld),
// clip b = the first lengths[b] samples of row b.
//
// Host side.  The clips' lengths (and whatever else a kernel needs per clip) travel as kernel arguments, at most kMax clips per set of
// launches: for_clip_slices cuts [0, B) into slices [b0, b0 + nb), narrow_clip_lengths fills a slice's length array and returns its
// longest clip, slice_rows moves a row pointer to the slice's first row.  What the entry points check of the lengths before any launch
// is check_clip_lengths (api.cpp).
//
// Device side, the element-wise passes (mix.hip, effects.hip): one grid over the batch, blockIdx.y = clip, blockIdx.x = chunk of
// kClipChunk samples of it.  A thread's samples are 16-byte groups of G = 16 / sizeof(T) samples (4 floats, 2 doubles) at the
// ROW-RELATIVE indices c0 + G (tid + 256 k): whatever a chunk sums, it sums the same samples in the same order at any row address, so a
// clip's result does not depend on the batch, the row stride or the alignment.  A group is ONE 16-byte access when the row's base is
// 16-byte aligned and the group lies inside the row; the groups of a misaligned row, and the tail group of a clip, go sample by sample.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace vfx {

constexpr int kClipChunk = 4096;  // samples of a clip per workgroup; mix.hip's float64 level sums are per chunk, combined in index order

// ---------------------------------------------------------------------------------------------
// host: slices of at most kMax clips
// ---------------------------------------------------------------------------------------------
template <int kMax, typename F>
inline void for_clip_slices(int B, F&& launch) {  // launch(b0, nb), 1 <= nb <= kMax
  for (int b0 = 0; b0 < B; b0 += kMax) launch(b0, std::min(B - b0, kMax));
}

// len[i] = lengths[b0 + i] for i < nb (Int is int, or int64_t for ResampleArgs); -> the longest of them
template <typename Int>
inline int64_t narrow_clip_lengths(const int64_t* lengths, int b0, int nb, Int* len) {
  int64_t nmax = 0;
  for (int i = 0; i < nb; ++i) {
    len[i] = (Int)lengths[b0 + i];
    nmax = std::max(nmax, lengths[b0 + i]);
  }
  return nmax;
}

// row b0 of a (clips, ld) array; NULL stays NULL.  The untyped forms take the element size.
template <typename T>
inline T* slice_rows(T* base, int b0, int64_t ld) {
  return base ? base + (int64_t)b0 * ld : nullptr;
}
inline const void* slice_rows(const void* base, int b0, int64_t ld, size_t esz) {
  return base ? static_cast<const char*>(base) + (size_t)b0 * ld * esz : nullptr;
}
inline void* slice_rows(void* base, int b0, int64_t ld, size_t esz) {
  return base ? static_cast<char*>(base) + (size_t)b0 * ld * esz : nullptr;
}

// ---------------------------------------------------------------------------------------------
// device: 16-byte sample groups, and the peak of a clip as a bit pattern
// ---------------------------------------------------------------------------------------------
template <typename T>
struct ClipType;
template <>
struct ClipType<float> {
  using Bits = unsigned;
  static __device__ __forceinline__ Bits abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
  static __device__ __forceinline__ float from_bits(Bits u) { return __uint_as_float(u); }
};
template <>
struct ClipType<double> {
  using Bits = unsigned long long;
  static __device__ __forceinline__ Bits abs_bits(double v) { return (Bits)__double_as_longlong(v) & 0x7fffffffffffffffull; }
  static __device__ __forceinline__ double from_bits(Bits u) { return __longlong_as_double((long long)u); }
};

template <typename T>
struct alignas(16) ClipGroup {
  T v[16 / sizeof(T)];
};

__device__ __forceinline__ bool clip_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// samples [j, j + G) of a row of n samples, j a multiple of G; zeros at and past n (bit pattern 0: no peak, and the callers test
// j + e < n before they use one)
template <typename T>
__device__ __forceinline__ void clip_load(const T* row, bool vec, int64_t j, int64_t n, T (&v)[16 / sizeof(T)]) {
  constexpr int G = 16 / sizeof(T);
  if (vec && j + G <= n) {
    const ClipGroup<T> q = *reinterpret_cast<const ClipGroup<T>*>(row + j);
#pragma unroll
    for (int e = 0; e < G; ++e) v[e] = q.v[e];
  } else {
#pragma unroll
    for (int e = 0; e < G; ++e) v[e] = j + e < n ? row[j + e] : T(0);
  }
}

// N values into a row of ld, from index j on (j a multiple of 16 / sizeof(T)), in 16-byte groups where they are whole and aligned
template <typename T, int N>
__device__ __forceinline__ void clip_store(T* row, bool vec, int64_t j, int64_t ld, const T (&v)[N]) {
  constexpr int G = 16 / sizeof(T);
  static_assert(N % G == 0, "whole groups");
#pragma unroll
  for (int g = 0; g < N; g += G) {
    if (vec && j + g + G <= ld) {
      ClipGroup<T> q;
#pragma unroll
      for (int e = 0; e < G; ++e) q.v[e] = v[g + e];
      *reinterpret_cast<ClipGroup<T>*>(row + j + g) = q;
    } else {
#pragma unroll
      for (int e = 0; e < G; ++e)
        if (j + g + e < ld) row[j + g + e] = v[g + e];
    }
  }
}

// the value one lane below within the 16-lane row (row_shr:1); lane 0 of a row gets 0.  What hands a sample from one section of a
// skewed cascade to the next (sosfilt.hip, chain.hip).
__device__ inline double row_shr1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// atomicMax(dst, the workgroup's largest `peak`) -- abs_bits patterns: order-independent, a NaN lands above every finite value, as
// np.max gives NaN.  The wave's max in registers, the workgroup's through LDS, then ONE atomic per workgroup, none for a zero: the
// atomics of a clip all land on one address (and those of 16 clips on one cache line), where they take their turns.  Every thread
// of the workgroup must come here (it holds a barrier); `slots` is LDS of the caller's, one set per call -- or a barrier between
// two calls on the same set.
template <int kThreads, typename Bits>
__device__ __forceinline__ void clip_commit_peak(Bits peak, Bits* dst, Bits (&slots)[kThreads / 64]) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) peak = max(peak, (Bits)__shfl_xor(peak, d));
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = peak;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) peak = max(peak, slots[w]);
    if (peak) atomicMax(dst, peak);
  }
}

}  // namespace vfx
