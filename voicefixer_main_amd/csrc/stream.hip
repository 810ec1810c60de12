// stream.hip -- the device side of a streaming session (vfx_stream_*): per-slot rings and the kernels that move samples between
// them and the caller's packed buffers / chunk batches.  Every position is worked out on the host (stream_sched.cpp) and reaches a
// kernel as a small table in its arguments, as k_set_frames takes its counts: no kernel reads a length another kernel wrote, and a
// table needs no staging buffer that a later call could overwrite.  A launch takes kStreamRows rows (kStreamOlaRows slots for the
// overlap-add stitch); longer tables go in several launches.
//
// All four are HBM-bound copies of a few rows; the cost that matters is launches per step (push + gather + stitch).
#include <hip/hip_runtime.h>

#include "stream.h"

namespace vfx {

typedef float sf32x4 __attribute__((ext_vector_type(4)));

static inline int blocks_of(int64_t n, int per) { return (int)((n + per - 1) / per); }

struct CopyTable {
  StreamCopyRow r[kStreamRows];
};
struct GatherTable {
  StreamGatherRow r[kStreamRows];
};
struct OlaTable {
  StreamOlaRow r[kStreamOlaRows];
};
struct BoxTable {
  StreamBoxRow r[kStreamRows];
};

// packed[off + i] <-> ring[slot][(pos + i) % cap], i < count <= cap.  TO_RING: push; else pop.
template <bool TO_RING>
__global__ void k_stream_copy(float* __restrict__ ring, int cap, float* __restrict__ packed, CopyTable t) {
  const StreamCopyRow r = t.r[blockIdx.y];
  float* const rb = ring + (int64_t)r.slot * cap;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < r.count; i += (int64_t)gridDim.x * 256) {
    int64_t c = r.pos + i;
    if (c >= cap) c -= cap;
    if (TO_RING)
      rb[c] = packed[r.off + i];
    else
      packed[r.off + i] = rb[c];
  }
}

// chunks[row][i] = x_slot[start + i] read from the slot's ring (cell pos + i, wrapping), zero outside [0, valid_end).
// One thread per 4 consecutive samples.  VEC: capacity and row length are multiples of 4 and both bases 16-byte aligned; a row whose
// start is a multiple of 4 then lies on the 16-byte grid of the ring, no vector straddles the wrap, and it moves 16 bytes per lane
// as k_chunk_gather does.  Every other row takes the scalar path.
template <bool VEC>
__global__ void k_stream_gather(const float* __restrict__ ring, int cap, int row_len, float* __restrict__ chunks, GatherTable t) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= row_len) return;
  const StreamGatherRow r = t.r[blockIdx.y];
  const float* const rb = ring + (int64_t)r.slot * cap;
  float* const dst = chunks + (int64_t)blockIdx.y * row_len + i;
  const int64_t n = r.start + i;
  int64_t c = r.pos + i;   // pos < cap and i < row_len <= cap: one wrap at most
  if (c >= cap) c -= cap;
  if (VEC && (r.start & 3) == 0) {
    sf32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n >= 0 && n + 4 <= r.valid_end) {
      v = *reinterpret_cast<const sf32x4*>(rb + c);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e >= 0 && n + e < r.valid_end) v[e] = rb[c + e];   // c % 4 == 0 and cap % 4 == 0: c + e < cap
    }
    *reinterpret_cast<sf32x4*>(dst) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i + e >= row_len) break;
      int64_t ce = c + e;
      if (ce >= cap) ce -= cap;
      dst[e] = (n + e >= 0 && n + e < r.valid_end) ? rb[ce] : 0.f;
    }
  }
}

// One term of the stitched sum.  k_chunk_ola's `acc += window ? f * window[i] : f * scale` compiles, for gfx950 under the Makefile's
// flags, to ONE v_fmac_f32 that both branches share (the branch only picks the multiplier), so the product is never rounded on
// its own: this is that instruction spelled out.
__device__ __forceinline__ float stream_term(float f, const float* __restrict__ window, float scale, int i, float acc) {
  return __fmaf_rn(f, window ? window[i] : scale, acc);
}

// Overlap-add stitch: a gather per stream position n of a slot's span -- the stored partial sum (cells below prior_end), then this
// step's chunks of the slot in ascending k.  Final positions go to the output ring, the others to the OTHER half of the slot's
// accumulator (a thread never writes a cell another thread of this launch reads).
__global__ void k_stream_ola(const float* __restrict__ frames, const float* __restrict__ window, float scale, int W, int H,
                             float* __restrict__ acc, float* __restrict__ out, int cap_out, OlaTable t) {
  const StreamOlaRow r = t.r[blockIdx.y];
  const int64_t n = r.span0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= r.span1) return;
  const int cell = (int)(n % W);
  const float* const rd = acc + ((int64_t)r.slot * 2 + r.parity) * W;
  float* const wr = acc + ((int64_t)r.slot * 2 + (r.parity ^ 1)) * W;
  float sum = n < r.prior_end ? rd[cell] : 0.f;
  const int64_t lo = n / H + 1, hi = (n + W) / H;   // the chunks [kH - W, kH) that hold n
  const int64_t ka = lo > r.k0 ? lo : r.k0, kb = hi < r.k0 + r.nk - 1 ? hi : r.k0 + r.nk - 1;
  for (int64_t k = ka; k <= kb; ++k) {
    const int i = (int)(n + W - k * H);
    sum = stream_term(frames[((int64_t)r.row0 + (k - r.k0)) * W + i], window, scale, i, sum);
  }
  if (n >= r.final_end)
    wr[cell] = sum;
  else if (n < r.out_limit)
    out[(int64_t)r.slot * cap_out + n % cap_out] = sum;
}

// Boxcar stitch: the kept part of each row, times the window, to the output ring (k_chunk_ola at hop = win: one term per sample).
__global__ void k_stream_box(const float* __restrict__ frames, int row_len, const float* __restrict__ window, float scale,
                             float* __restrict__ out, int cap_out, BoxTable t) {
  const StreamBoxRow r = t.r[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= r.count) return;
  const float f = frames[(int64_t)r.row * row_len + r.off + j];
  out[(int64_t)r.slot * cap_out + (r.n0 + j) % cap_out] = stream_term(f, window, scale, j, 0.f);
}

// ---------------------------------------------------------------------------------------------
// launches: a table of any length, kStreamRows (kStreamOlaRows) rows per launch
// ---------------------------------------------------------------------------------------------
void launch_stream_copy(bool to_ring, float* ring, int cap, float* packed, const std::vector<StreamCopyRow>& rows, hipStream_t s) {
  for (size_t first = 0; first < rows.size(); first += kStreamRows) {
    CopyTable t{};
    const int n = (int)std::min<size_t>(kStreamRows, rows.size() - first);
    int64_t most = 0;
    for (int i = 0; i < n; ++i) {
      t.r[i] = rows[first + i];
      most = std::max(most, t.r[i].count);
    }
    if (most <= 0) continue;
    const dim3 grid(std::min(blocks_of(most, 256), 1024), n);
    if (to_ring)
      hipLaunchKernelGGL(k_stream_copy<true>, grid, dim3(256), 0, s, ring, cap, packed, t);
    else
      hipLaunchKernelGGL(k_stream_copy<false>, grid, dim3(256), 0, s, ring, cap, packed, t);
    VFX_HIP(hipGetLastError());
  }
}

void launch_stream_gather(const float* ring, int cap, int row_len, float* chunks, const std::vector<StreamGatherRow>& rows,
                          hipStream_t s) {
  const bool vec = cap % 4 == 0 && row_len % 4 == 0 && reinterpret_cast<uintptr_t>(ring) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(chunks) % 16 == 0;
  for (size_t first = 0; first < rows.size(); first += kStreamRows) {
    GatherTable t{};
    const int n = (int)std::min<size_t>(kStreamRows, rows.size() - first);
    for (int i = 0; i < n; ++i) t.r[i] = rows[first + i];
    const dim3 grid(blocks_of(row_len, 1024), n);
    float* const dst = chunks + (int64_t)first * row_len;
    if (vec)
      hipLaunchKernelGGL(k_stream_gather<true>, grid, dim3(256), 0, s, ring, cap, row_len, dst, t);
    else
      hipLaunchKernelGGL(k_stream_gather<false>, grid, dim3(256), 0, s, ring, cap, row_len, dst, t);
    VFX_HIP(hipGetLastError());
  }
}

void launch_stream_ola(const float* frames, const float* window, float scale, int W, int H, float* acc, float* out, int cap_out,
                       const std::vector<StreamOlaRow>& rows, hipStream_t s) {
  for (size_t first = 0; first < rows.size(); first += kStreamOlaRows) {
    OlaTable t{};
    const int n = (int)std::min<size_t>(kStreamOlaRows, rows.size() - first);
    int64_t most = 0;
    for (int i = 0; i < n; ++i) {
      t.r[i] = rows[first + i];
      most = std::max(most, t.r[i].span1 - t.r[i].span0);
    }
    if (most <= 0) continue;
    hipLaunchKernelGGL(k_stream_ola, dim3(blocks_of(most, 256), n), dim3(256), 0, s, frames, window, scale, W, H, acc, out, cap_out, t);
    VFX_HIP(hipGetLastError());
  }
}

void launch_stream_box(const float* frames, int row_len, const float* window, float scale, float* out, int cap_out,
                       const std::vector<StreamBoxRow>& rows, hipStream_t s) {
  for (size_t first = 0; first < rows.size(); first += kStreamRows) {
    BoxTable t{};
    const int n = (int)std::min<size_t>(kStreamRows, rows.size() - first);
    int64_t most = 0;
    for (int i = 0; i < n; ++i) {
      t.r[i] = rows[first + i];
      most = std::max(most, t.r[i].count);
    }
    if (most <= 0) continue;
    hipLaunchKernelGGL(k_stream_box, dim3(blocks_of(most, 256), n), dim3(256), 0, s, frames, row_len, window, scale, out, cap_out, t);
    VFX_HIP(hipGetLastError());
  }
}

}  // namespace vfx
