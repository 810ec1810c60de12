// stft_wave.h -- the wave-level arithmetic of the STFT front end that more than one kernel file evaluates: the 1024-point complex FFT
// of one wave, the reflect-padded frame load, the real-FFT untangle and the clamped magnitude.  stft.hip (k_stft_mel, k_istft,
// k_stft_lowpass, k_stft_splice), losses.hip (k_pair_stft_l1), band.hip (k_band_energy) and splice.hip (k_pair_band_power) include it; a
// magnitude is the same float32 in all of them.
#pragma once
#include "vfx_internal.h"

// Floating-point contraction is OFF in this file: every fused multiply-add below is written as fmaf.  Left to itself the compiler
// fuses a * b + c where it sees fit, and what it sees depends on the kernel around the expression (which operations the
// vectoriser paired, what a product feeds into): the same source rounds differently in two kernels.  k_stft_lowpass has to give
// bit for bit what k_stft_mel followed by k_istft give, so the arithmetic they share is pinned down here, once.
#pragma clang fp contract(off)

namespace vfx {

constexpr int NFFT = 2048;
constexpr int NC = NFFT / 2;     // complex FFT length
constexpr int NBINS = NC + 1;    // 1025
constexpr int NMEL = 128;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

// In-place (register) radix-4 butterfly.  SIGN = -1: forward (e^{-i}), +1: inverse.
template <int SIGN>
__device__ __forceinline__ void fft4(float2& v0, float2& v1, float2& v2, float2& v3) {
  const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y);
  const float2 a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
  const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y);
  const float2 d = make_float2(v1.x - v3.x, v1.y - v3.y);
  // forward: d * (-i) = (d.y, -d.x);  inverse: d * (+i) = (-d.y, d.x)
  const float2 a3 = SIGN < 0 ? make_float2(d.y, -d.x) : make_float2(-d.y, d.x);
  v0 = make_float2(a0.x + a2.x, a0.y + a2.y);
  v1 = make_float2(a1.x + a3.x, a1.y + a3.y);
  v2 = make_float2(a0.x - a2.x, a0.y - a2.y);
  v3 = make_float2(a1.x - a3.x, a1.y - a3.y);
}

// ---- wave-level 1024-point complex FFT -----------------------------------------------------------------------------------
// ONE wave transforms a frame: 64 lanes x 16 points, Stockham passes of radix 16, 16, 4 (the 16-point butterfly = two
// radix-4 stages in registers), the three exchanges through the wave's own LDS buffer -- no block barrier anywhere: a
// wave's LDS operations execute in order, so a `wave_sync()` (compiler fence) between a store and the loads of other lanes'
// data is all it takes.  The 256-thread form (five radix-4 passes, two block barriers each, one frame per workgroup at a
// time) kept the chip at a handful of frames in flight per CU: 7 us per frame of barrier and LDS latency for 0.3 us of
// arithmetic.
constexpr int ZP = NC + NC / 16 + 1;  // float2 per wave buffer: one pad element per 16 (conflict-free strided access) + 1 (below)
__device__ __forceinline__ int zpad(int i) { return i + (i >> 4); }
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// 16-point DFT in registers, n = 4a + b -> k = c + 4d: radix-4 over a, twiddle W16^(bc), radix-4 over b.
// On return X[k] sits in v[4 (k & 3) + (k >> 2)] (see out16()).
template <int SIGN>
__device__ __forceinline__ void fft16(float2 (&v)[16]) {
#pragma unroll
  for (int b = 0; b < 4; ++b) fft4<SIGN>(v[b], v[4 + b], v[8 + b], v[12 + b]);  // v[4c + b] = Y_b[c]
  constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
  constexpr float s = SIGN < 0 ? -1.f : 1.f;  // W16^m = cos(2 pi m / 16) + s i sin(2 pi m / 16)
  auto tw = [&](float2& x, float c, float sn) __attribute__((always_inline)) { x = cmul(x, make_float2(c, s * sn)); };
  tw(v[4 * 1 + 1], C1, S1);    // m = 1
  tw(v[4 * 1 + 2], R2, R2);    // m = 2
  tw(v[4 * 1 + 3], S1, C1);    // m = 3
  tw(v[4 * 2 + 1], R2, R2);    // m = 2
  v[4 * 2 + 2] = SIGN < 0 ? make_float2(v[10].y, -v[10].x) : make_float2(-v[10].y, v[10].x);  // m = 4: -+ i
  tw(v[4 * 2 + 3], -R2, R2);   // m = 6
  tw(v[4 * 3 + 1], S1, C1);    // m = 3
  tw(v[4 * 3 + 2], -R2, R2);   // m = 6
  tw(v[4 * 3 + 3], -C1, -S1);  // m = 9
#pragma unroll
  for (int c = 0; c < 4; ++c) fft4<SIGN>(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);  // v[4c + d] = X[c + 4d]
}
__device__ __forceinline__ constexpr int out16(int k) { return 4 * (k & 3) + (k >> 2); }

// In: v[r] = x[lane + 64 r].  Out: v[m] = X[lane + 64 m] (natural order).  `zw` = this wave's LDS buffer (ZP float2), `twl` =
// the workgroup's LDS copy of e^{-2 pi i m / 1024} (conjugated here for the inverse).
template <int SIGN>
__device__ __forceinline__ void wfft1024(float2 (&v)[16], float2* zw, const float2* twl, int lane) {
  auto twid = [&](int idx) __attribute__((always_inline)) {
    float2 w = twl[idx];
    if (SIGN > 0) w.y = -w.y;
    return w;
  };
  // (padded positions written out: i + (i >> 4) is linear in r for every access pattern below, so each is one base address
  // plus an immediate offset)
  // pass 1: radix 16, Ns = 1 (no twiddles): out[16 lane + r] -> 17 lane + r
  fft16<SIGN>(v);
  float2* const w1 = zw + 17 * lane;
#pragma unroll
  for (int r = 0; r < 16; ++r) w1[r] = v[out16(r)];
  wave_sync();
  // pass 2: radix 16, Ns = 16: in[lane + 64 r] * W256^(k r), k = lane mod 16;  out[16 (lane - k) + k + 16 r]
  const int k = lane & 15;
  const float2* const r2 = zw + lane + (lane >> 4);  // in[lane + 64 r] -> + 68 r
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = r2[68 * r];
#pragma unroll
  for (int r = 1; r < 16; ++r) v[r] = cmul(v[r], twid(4 * k * r));
  wave_sync();
  fft16<SIGN>(v);
  float2* const w2 = zw + 17 * (lane - k) + k;  // out[16 (lane - k) + k + 16 r] -> + 17 r
#pragma unroll
  for (int r = 0; r < 16; ++r) w2[17 * r] = v[out16(r)];
  wave_sync();
  // pass 3: radix 4, Ns = 256: four butterflies per lane, j = lane + 64 q: in[j + 256 r] * W1024^(j r) -> X[j + 256 r]
  float2 u[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane + 64 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) u[4 * q + r] = r2[68 * q + 272 * r];  // in[j + 256 r]
#pragma unroll
    for (int r = 1; r < 4; ++r) u[4 * q + r] = cmul(u[4 * q + r], twid(j * r));
    fft4<SIGN>(u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]);
  }
  wave_sync();  // every lane is done reading zw: the caller may overwrite it
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[q + 4 * r] = u[4 * q + r];  // X[lane + 64 (q + 4 r)]
}

// base[idx] with a wave-uniform base and a 32-bit BYTE offset: the scalar-base addressing mode (one VGPR per address)
__device__ __forceinline__ float ldg32(const float* base, unsigned idx) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + 4u * idx);
}

__device__ __forceinline__ int reflect_index(int i, int L) {
  i = i < 0 ? -i : i;
  return i >= L ? 2 * (L - 1) - i : i;
}

// The sixteen sample pairs (x[2n], x[2n+1]), n = lane + 64 r, of the reflect-padded frame t.  `x` is wave-uniform (a scalar
// base): every load is base + one 32-bit lane offset.
__device__ __forceinline__ void load_frame(const float* __restrict__ x, int L, int t, int hop, int lane, float2 (&out)[16]) {
  const int base = t * hop - NFFT / 2;
  if (base >= 0 && base + NFFT <= L) {  // wave-uniform: an interior frame
    const unsigned o = (unsigned)(base + 2 * lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = make_float2(ldg32(x, o + 128u * r), ldg32(x, o + 128u * r + 1u));
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int g = base + 2 * (lane + 64 * r);
      out[r] = make_float2(ldg32(x, (unsigned)reflect_index(g, L)), ldg32(x, (unsigned)reflect_index(g + 1, L)));
    }
  }
}

constexpr int STFT_WAVES = 4;  // waves per workgroup: each walks its own frames

// e^{-2 pi i (lane + 64 m) / 2048} = e^{-2 pi i lane / 2048} * e^{-2 pi i m / 32}: the lane's own factor (one table read per
// wave) times a compile-time constant -- no table read per bin
__device__ __forceinline__ float2 rtw_of(float2 lane_w, int m) {
  constexpr float C[16] = {1.f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f, 0.70710678118654752f,
                           0.55557023301960218f, 0.38268343236508977f, 0.19509032201612825f, 0.f, -0.19509032201612825f,
                           -0.38268343236508977f, -0.55557023301960218f, -0.70710678118654752f, -0.83146961230254524f,
                           -0.92387953251128674f, -0.98078528040323043f};
  constexpr float S[16] = {0.f, 0.19509032201612825f, 0.38268343236508977f, 0.55557023301960218f, 0.70710678118654752f,
                           0.83146961230254524f, 0.92387953251128674f, 0.98078528040323043f, 1.f, 0.98078528040323043f,
                           0.92387953251128674f, 0.83146961230254524f, 0.70710678118654752f, 0.55557023301960218f,
                           0.38268343236508977f, 0.19509032201612825f};
  return cmul(lane_w, make_float2(C[m], -S[m]));
}

// v[m] = A[lane + 64 m] (natural order) -> pn[m] = A[1024 - (lane + 64 m)], through the wave's LDS buffer: what the real-FFT
// untangle (A = Z) and the Hermitian pack (A = X) pair a bin with.
// A[1024 - (lane + 64 m)] = A[(64 - lane) + 64 (15 - m)]; lane 0: A[64 (16 - m)], and its m = 0 reads A[1024] from the spare element
// behind the buffer (zw[ZP - 1]): whatever the caller put there, or the caller overwrites pn[0].  On return zw is free.
__device__ __forceinline__ void mirror_bins(const float2 (&v)[16], float2 (&pn)[16], float2* zw, int lane) {
  float2* const nat = zw + lane + (lane >> 4);  // A[lane + 64 m] -> + 68 m
#pragma unroll
  for (int m = 0; m < 16; ++m) nat[68 * m] = v[m];
  wave_sync();
  const int jp = 64 - lane;
  const float2* const par = lane == 0 ? zw + 68 : zw + jp + (jp >> 4);
#pragma unroll
  for (int m = 0; m < 16; ++m) pn[m] = par[68 * (15 - m)];
  wave_sync();
}

// real-FFT untangle of one bin: X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[N-k]) / 2, O = (Z[k] - conj Z[N-k]) / (2i), and its
// magnitude, clamped on the POWER (fDomainHelper.py:62); v_sqrt_f32 (1 ulp) instead of the IEEE expansion
__device__ __forceinline__ void untangle_bin(float2 zk, float2 znk, float2 wk, float eps, float& re, float& im, float& mag) {
  const float2 o = make_float2(0.5f * (zk.y + znk.y), -0.5f * (zk.x - znk.x));
  const float2 wo = cmul(wk, o);
  re = fmaf(0.5f, zk.x + znk.x, wo.x);  // E + W^k O
  im = fmaf(0.5f, zk.y - znk.y, wo.y);
  mag = __builtin_amdgcn_sqrtf(fmaxf(fmaf(im, im, re * re), eps));
}

// ---- the frame walk of the kernels that keep no spectrum (k_pair_stft_l1, k_band_energy) ------------------------------------------
// v = the frame's sample pairs times the window: the first step of k_stft_mel's frame walk
__device__ __forceinline__ void window_frame(const float2 (&xin)[16], const float2* wl, int lane, float2 (&v)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float2 ww = wl[lane + 64 * r];
    v[r] = make_float2(xin[r].x * ww.x, xin[r].y * ww.y);
  }
}

// The windowed frame v -> mag[m] = |X[lane + 64 m]|, top = |X[1024]| (lane 0; 0 elsewhere): the transform, the mirror and the untangle
// in k_stft_mel's order, with its expressions.  On return the wave's LDS buffer is free.
__device__ __forceinline__ void frame_magnitudes(float2 (&v)[16], float2* zw, const float2* twl, float2 rtw_lane, int lane, float eps,
                                                 float (&mag)[16], float& top) {
  wfft1024<-1>(v, zw, twl, lane);
  float2 zn[16];
  mirror_bins(v, zn, zw, lane);
  if (lane == 0) zn[0] = v[0];  // Z[1024] = Z[0]
  __builtin_amdgcn_sched_barrier(0);
  float re, im;
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    untangle_bin(v[m], zn[m], rtw_of(rtw_lane, m), eps, re, im, mag[m]);
    if ((m & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // four bins at a time, as in the forward kernel
  }
  top = 0.f;
  if (lane == 0) untangle_bin(v[0], zn[0], make_float2(-1.f, 0.f), eps, re, im, top);  // W^1024 = -1
}

}  // namespace vfx
