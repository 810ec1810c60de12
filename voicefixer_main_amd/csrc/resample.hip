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
  for (int b0 = 0; b0 < B; b0 += kResampleMaxClips) {  // the clips' lengths travel as kernel arguments, kResampleMaxClips per launch
    const int nbat = std::min(B - b0, kResampleMaxClips);
    a.x = x + (int64_t)b0 * ldx;
    a.y = y + (int64_t)b0 * ldy;
    for (int i = 0; i < nbat; ++i) {
      a.lens_in[i] = lens_in[b0 + i];
      a.lens_out[i] = resample_out_len(lens_in[b0 + i], p);
    }
    const dim3 grid((unsigned)nb, (unsigned)nbat);
    if (p.R == 4)
      hipLaunchKernelGGL(k_resample_poly<4>, grid, dim3(256), (size_t)lds_floats * 4, s, a);
    else if (p.R == 2)
      hipLaunchKernelGGL(k_resample_poly<2>, grid, dim3(256), (size_t)lds_floats * 4, s, a);
    else
      hipLaunchKernelGGL(k_resample_poly<1>, grid, dim3(256), (size_t)lds_floats * 4, s, a);
    VFX_HIP(hipGetLastError());
  }
}

}  // namespace vfx
