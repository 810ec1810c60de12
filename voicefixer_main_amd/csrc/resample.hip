// resample.hip -- batched polyphase FIR resampler (gfx950), bit-identical to scipy.signal.resample_poly on float32 input.
//
// resample_poly(x, up, down) with its default Kaiser(5.0) filter, after reducing up / down by their gcd (M = max(up, down),
// hl = 10 * M, the caller's taps h = float32(firwin(2 hl + 1, 1 / M)) * float32(up)) computes, per output n < ceil(n_in up / down):
//
//   y[n] = sum over ascending k, 0 <= k < n_in, 0 <= n down + hl - k up <= 2 hl :  acc = fl32(acc + fl32(x[k] * h[n down + hl - k up]))
//
// (scipy's upfirdn: one float32 multiply, then one float32 add per term, no FMA; n_pre_pad / n_pre_remove add up to hl).  The kernel
// keeps that order with contraction off, so its outputs are those of resample_poly down to the last bit (tests/test_gpu_resample.py).
//
// One lane per output, R outputs per lane 256 apart: a workgroup owns 256 R consecutive outputs of one clip, stages the taps and
// the input span those outputs need in LDS once, then each lane walks its phase (the tap index steps down by `up` as k rises).
#include "clip_batch.h"
#include "vfx_internal.h"

namespace vfx {

static inline int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

__host__ __device__ inline int64_t floor_div(int64_t a, int64_t b) {  // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

constexpr int kResampleLdsBytes = 65536;

// floats of LDS a workgroup of `R` outputs per lane needs: the taps (padded to 4) + the widest input span of 256 R outputs
static int64_t resample_lds_floats(int up, int down, int R) {
  const int64_t hl = 10 * (int64_t)std::max(up, down);
  const int64_t taps = (2 * hl + 1 + 3) / 4 * 4;
  const int64_t span = ((int64_t)(256 * R - 1) * down + 2 * hl) / up + 2;
  return taps + span;
}

bool resample_reduce(int64_t up, int64_t down, ResamplePair* out) {
  if (up <= 0 || down <= 0) return false;
  const int64_t g = gcd64(up, down);
  up /= g;
  down /= g;
  if (up > (1 << 20) || down > (1 << 20)) return false;
  out->up = (int)up;
  out->down = (int)down;
  out->hl = 10 * (int)std::max(up, down);
  out->R = 0;
  if (up == down) return true;  // the same rate: no filter (resample_poly returns a copy)
  for (int R : {4, 2, 1})
    if (resample_lds_floats(out->up, out->down, R) * 4 <= kResampleLdsBytes) {
      out->R = R;
      break;
    }
  return true;
}

int64_t resample_out_len(int64_t n_in, const ResamplePair& p) { return ceil_div(n_in * p.up, p.down); }

void resample_window(int64_t n_in, const ResamplePair& p, int64_t o0, int64_t n, int64_t* k0, int64_t* k1) {
  const int64_t o1 = std::min(o0 + n, resample_out_len(n_in, p));  // outputs at or past the clip's end are zeros: they need nothing
  *k0 = *k1 = 0;
  if (o1 <= o0) return;
  if (p.up == p.down) {  // the same rate: a copy
    *k0 = o0;
    *k1 = o1;
    return;
  }
  const int64_t lo = std::max<int64_t>(0, ceil_div(o0 * p.down - p.hl, p.up));
  const int64_t hi = std::min<int64_t>(n_in, floor_div((o1 - 1) * p.down + p.hl, p.up) + 1);
  if (hi > lo) {
    *k0 = lo;
    *k1 = hi;
  }
}

template <int R>
__global__ __launch_bounds__(256) void k_resample_poly(const ResampleArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int up = a.up, down = a.down, hl = a.hl;
  const int ntaps = 2 * hl + 1;
  float* taps_s = smem;
  float* xs = smem + ((ntaps + 3) & ~3);
  const int64_t lin = a.lens_in[b], lout = a.lens_out[b];
  const int64_t n0 = a.o0 + (int64_t)blockIdx.x * (256 * R);
  const int64_t nlast = min(n0 + 256 * R, a.o0 + a.n_out) - 1;
  // the input span the block's outputs need, inside the caller's window and the clip (outside: scipy's zero padding)
  const int64_t s_lo = max(ceil_div(n0 * down - hl, up), max((int64_t)0, a.x0));
  const int64_t s_hi = min(min(floor_div(nlast * down + hl, up), min(lin, a.x0 + a.Lx) - 1), s_lo + a.span_max - 1);
  for (int i = tid; i < ntaps; i += 256) taps_s[i] = a.taps[i];
  const float* xb = a.x + (int64_t)b * a.ldx - a.x0;
  for (int64_t k = s_lo + tid; k <= s_hi; k += 256) xs[k - s_lo] = xb[k];
  __syncthreads();
  float* yb = a.y + (int64_t)b * a.ldy - a.o0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int64_t n = n0 + j * 256 + tid;
    if (n > nlast) break;
    float acc = 0.f;
    if (n < lout) {
      const int64_t t = n * down + hl;
      const int64_t k_lo = max(ceil_div(t - 2 * hl, up), s_lo);
      const int64_t k_hi = min(floor_div(t, up), s_hi);
      const float* xp = xs + (k_lo - s_lo);
      int hi = (int)(t - k_lo * up);  // in [0, 2 hl]: k >= ceil((t - 2 hl) / up) and k <= floor(t / up)
      const int cnt = (int)(k_hi - k_lo + 1);
      for (int c = 0; c < cnt; ++c) {
        const float p = xp[c] * taps_s[hi];  // two roundings, never an FMA (contract off): scipy's order and arithmetic
        acc = acc + p;
        hi -= up;
      }
    }
    yb[n] = acc;
  }
}

void launch_resample(const float* x, int B, int64_t ldx, int64_t x0, int64_t Lx, const int64_t* lens_in, const ResamplePair& p,
                     const float* taps, float* y, int64_t ldy, int64_t o0, int64_t n_out, hipStream_t s) {
  VFX_CHECK(p.R > 0, "resample: the filter of %d/%d does not fit the LDS budget", p.up, p.down);
  const int64_t lds_floats = resample_lds_floats(p.up, p.down, p.R);
  const int64_t per_block = 256 * (int64_t)p.R;
  const int64_t nb = (n_out + per_block - 1) / per_block;
  VFX_CHECK(nb <= 0x7fffffff, "resample: output window too long");
  const void* fn = p.R == 4 ? reinterpret_cast<const void*>(k_resample_poly<4>)
                 : p.R == 2 ? reinterpret_cast<const void*>(k_resample_poly<2>)
                            : reinterpret_cast<const void*>(k_resample_poly<1>);
  static uint64_t attr_devices[3] = {0, 0, 0};
  if (first_use_on_current_device(attr_devices[p.R == 4 ? 2 : p.R - 1]))
    VFX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kResampleLdsBytes));
  ResampleArgs a{};
  a.taps = taps;
  a.ldx = ldx;
  a.x0 = x0;
  a.Lx = Lx;
  a.ldy = ldy;
  a.o0 = o0;
  a.n_out = n_out;
  a.up = p.up;
  a.down = p.down;
  a.hl = p.hl;
  a.span_max = (int)(lds_floats - (2 * (int64_t)p.hl + 1 + 3) / 4 * 4);
  for_clip_slices<kResampleMaxClips>(B, [&](int b0, int nbat) {
    a.x = slice_rows(x, b0, ldx);
    a.y = slice_rows(y, b0, ldy);
    narrow_clip_lengths(lens_in, b0, nbat, a.lens_in);
    for (int i = 0; i < nbat; ++i) a.lens_out[i] = resample_out_len(a.lens_in[i], p);
    const dim3 grid((unsigned)nb, (unsigned)nbat);
    if (p.R == 4)
      hipLaunchKernelGGL(k_resample_poly<4>, grid, dim3(256), (size_t)lds_floats * 4, s, a);
    else if (p.R == 2)
      hipLaunchKernelGGL(k_resample_poly<2>, grid, dim3(256), (size_t)lds_floats * 4, s, a);
    else
      hipLaunchKernelGGL(k_resample_poly<1>, grid, dim3(256), (size_t)lds_floats * 4, s, a);
    VFX_HIP(hipGetLastError());
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The per-clip form: a rate pair per clip, float32 or float64, max(up, down) up to kResampleEachMaxRate (1.3 M taps).  The same
// recurrence in the clip's dtype T; the taps stay in global memory (L2).  A call first scales the unscaled firwin g of each of its
// designs, h = fl_T(g T(up)) -- scipy's `h *= up` --, into a buffer of the handle that only grows (k_resample_each_taps), phase-major:
//
//   P[phi][j] = h[phi + j up],  0 <= phi < up, rows of J = 2 hl / up + 1
//
// With t = n down + hl = q up + phi, the tap of input k is h[t - k up] = P[phi][q - k]: as k rises a lane walks ONE row backwards,
// where the natural order would touch a cache line per tap.  The order of the sum, and so every bit of it, is the same either way
// (vfx_handle::rs_natural_taps keeps the natural order selectable for measurements).  One lane per output, kResampleEachBlock
// outputs of one clip per workgroup; the input is read from global memory as well (a block's span is short and contiguous, and for
// the down step its size has no bound that LDS could hold).
// ---------------------------------------------------------------------------------------------------------------------------------
bool resample_each_reduce(int64_t up, int64_t down, ResamplePair* out) {
  if (up <= 0 || down <= 0) return false;
  const int64_t g = gcd64(up, down);
  up /= g;
  down /= g;
  if (std::max(up, down) > kResampleEachMaxRate) return false;
  out->up = (int)up;
  out->down = (int)down;
  out->hl = 10 * (int)std::max(up, down);
  out->R = 0;
  return true;
}

template <typename T>
__global__ __launch_bounds__(256) void k_resample_each_taps(const T* __restrict__ g, T* __restrict__ P,
                                                            const ResampleEachDesign* __restrict__ designs, int natural) {
#pragma clang fp contract(off)
  const ResampleEachDesign d = designs[blockIdx.y];
  const T scale = (T)d.up;  // exact: up <= 65536
  for (int i = blockIdx.x * 256 + threadIdx.x; i < d.ntaps; i += gridDim.x * 256) {
    const int64_t at = natural ? (int64_t)i : (int64_t)(i % d.up) * d.J + i / d.up;  // i / up <= 2 hl / up = J - 1
    P[d.dst + at] = g[d.src + i] * scale;
  }
}

template <typename T>
__global__ __launch_bounds__(kResampleEachBlock) void k_resample_each(const T* __restrict__ x, const T* __restrict__ P, T* __restrict__ y,
                                                                      const ResampleEachClip* __restrict__ clips, int64_t n_out,
                                                                      int natural) {
#pragma clang fp contract(off)
  const ResampleEachClip c = clips[blockIdx.y];
  const int64_t n = (int64_t)blockIdx.x * kResampleEachBlock + threadIdx.x;
  if (n >= n_out) return;
  T acc = (T)0;
  if (n < c.len_out) {
    const T* xb = x + c.x_at;
    if (c.up == c.down) {  // the same rate: a copy (len_out = len_in)
      acc = xb[n];
    } else {
      const int64_t t = n * c.down + c.hl;  // < 2^63: n down < (len_in + 1) up
      const int64_t q = t / c.up;           // the one division of the output
      const int phi = (int)(t - q * c.up);
      const int jmax = (2 * c.hl - phi) / c.up;  // t - k up <= 2 hl  <=>  q - k <= jmax  (phi < up <= 2 hl)
      const int64_t k_lo = max(q - jmax, (int64_t)0);
      const int64_t k_hi = min(q, c.len_in - 1);  // t - k up >= 0  <=>  k <= q
      const int cnt = (int)max(k_hi - k_lo + 1, (int64_t)0);  // <= jmax + 1
      const T* xp = xb + k_lo;                                // k in [0, len_in)
      // the tap of k_lo + i is row phi's entry j - i, j = q - k_lo in [cnt - 1, jmax]; natural order: h[phi + (j - i) up] <= h[2 hl]
      const int64_t step = natural ? c.up : 1;
      const T* tp = P + c.taps_at + (natural ? (int64_t)phi : (int64_t)phi * c.J) + (q - k_lo) * step;
#pragma unroll 4
      for (int i = 0; i < cnt; ++i) {
        const T p = xp[i] * tp[-(int64_t)i * step];  // two roundings, never an FMA (contract off): scipy's order and arithmetic
        acc = acc + p;
      }
    }
  }
  y[c.y_at + n] = acc;
}

void launch_resample_each(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lens_in, const int* pair_index,
                          const ResamplePair* pairs, const void* taps, const int64_t* taps_at, int F, void* y, int64_t ldy, int64_t n_out,
                          hipStream_t s) {
  const size_t esize = x_f64 ? sizeof(double) : sizeof(float);
  const int natural = h->rs_natural_taps ? 1 : 0;
  const size_t designs_bytes = (size_t)F * sizeof(ResampleEachDesign), table_bytes = designs_bytes + (size_t)B * sizeof(ResampleEachClip);
  char* const host = h->rs_table.stage(h, table_bytes);
  ResampleEachDesign* const designs = reinterpret_cast<ResampleEachDesign*>(host);
  ResampleEachClip* const clips = reinterpret_cast<ResampleEachClip*>(host + designs_bytes);
  size_t elems = 0;
  int max_ntaps = 0;
  for (int f = 0; f < F; ++f) {
    const ResamplePair& p = pairs[f];
    ResampleEachDesign& d = designs[f];
    d = ResampleEachDesign{};
    d.up = p.up;
    d.J = 2 * p.hl / p.up + 1;
    d.ntaps = p.up == p.down ? 0 : 2 * p.hl + 1;  // the same rate: no filter, taps_at[f] is not read
    d.src = d.ntaps ? taps_at[f] : 0;
    d.dst = (int64_t)elems;
    if (d.ntaps) elems += ((size_t)p.up * d.J + 63) / 64 * 64;  // >= ntaps in either order: up J >= 2 hl + 1
    max_ntaps = std::max(max_ntaps, d.ntaps);
  }
  for (int b = 0; b < B; ++b) {
    const int f = pair_index[b];
    const ResamplePair& p = pairs[f];
    ResampleEachClip& c = clips[b];
    c = ResampleEachClip{};
    c.x_at = (int64_t)b * ldx;
    c.y_at = (int64_t)b * ldy;
    c.len_in = lens_in[b];
    c.len_out = ceil_div(lens_in[b] * p.up, p.down);
    c.taps_at = designs[f].dst;
    c.up = p.up;
    c.down = p.down;
    c.hl = p.hl;
    c.J = designs[f].J;
  }
  // the scaled taps of the call's designs: at most 21 * 65536 elements each (11 MB in float64), 128 designs
  char* const P = elems ? h->rs_taps.ensure(h, elems * esize, 0) : nullptr;
  const char* const dev = h->rs_table.upload(table_bytes, s);
  const ResampleEachDesign* const d_designs = reinterpret_cast<const ResampleEachDesign*>(dev);
  const ResampleEachClip* const d_clips = reinterpret_cast<const ResampleEachClip*>(dev + designs_bytes);
  const dim3 taps_grid((unsigned)std::min((max_ntaps + 255) / 256, 1024), (unsigned)F);
  const dim3 grid((unsigned)((n_out + kResampleEachBlock - 1) / kResampleEachBlock), (unsigned)B);  // the caller has bounded n_out
  if (x_f64) {
    if (max_ntaps)
      hipLaunchKernelGGL(k_resample_each_taps<double>, taps_grid, dim3(256), 0, s, static_cast<const double*>(taps),
                         reinterpret_cast<double*>(P), d_designs, natural);
    hipLaunchKernelGGL(k_resample_each<double>, grid, dim3(kResampleEachBlock), 0, s, static_cast<const double*>(x),
                       reinterpret_cast<const double*>(P), static_cast<double*>(y), d_clips, n_out, natural);
  } else {
    if (max_ntaps)
      hipLaunchKernelGGL(k_resample_each_taps<float>, taps_grid, dim3(256), 0, s, static_cast<const float*>(taps),
                         reinterpret_cast<float*>(P), d_designs, natural);
    hipLaunchKernelGGL(k_resample_each<float>, grid, dim3(kResampleEachBlock), 0, s, static_cast<const float*>(x),
                       reinterpret_cast<const float*>(P), static_cast<float*>(y), d_clips, n_out, natural);
  }
  VFX_HIP(hipGetLastError());
}

}  // namespace vfx
