// stft.hip -- fused STFT front-end / ISTFT back-end for gfx950.
//
// Forward (vfx_stft_mel): ONE WAVE per frame.  A wave walks F consecutive frames of one clip (F chosen so that the launch is
//   about one round of resident waves); four waves share a workgroup's tables -- the FFT twiddles, the periodic Hann window
//   and the non-zeros of the mel filterbank in LDS -- and nothing else: after the table fill there is no block barrier.
//   Per frame: reflect-padded frame x window  ->  1024-point complex FFT by the wave (64 lanes x 16 points: Stockham passes of
//   radix 16, 16, 4, three exchanges through the wave's own 8.7 KB of LDS)  ->  real-FFT untangle to 1025 bins  ->
//   mag = sqrt(max(re^2+im^2, eps)), cos = re/mag, sin = im/mag (FDomainHelper.spectrogram_phase,
//   tools/pytorch/modules/fDomainHelper.py:60-65)  ->  banded sparse mel projection from LDS (MelScale.forward,
//   tools/pytorch/mel_scale.py:52-64; the filterbank has 2018 non-zeros, 1..55 per band; a lane sums band `lane` and band
//   `127 - lane`)  ->  optional log10(max(.,1e-8)) (to_log, tools/pytorch/pytorch_util.py:157-159).  The samples of frame
//   t+1 are requested before the FFT of frame t.
//   The reference does the DFT as two conv1d(1->1025, k=2048) = 4.2 MMAC/frame; the FFT path needs 79 kflop/frame.  With
//   2276 B/frame of algorithmic traffic (441 new samples in, 128 mel out) the mel-only front-end is bound by VALU ISSUE, not
//   by HBM (35 flop/B against a ridge of 20): a wave64 instruction occupies its SIMD for four cycles and a frame is ~2300 of
//   them.  Measured (16 x 10 s): 65 us = 0.07 of the HBM roofline / 0.12 of the fp32 vector peak; the phase-emitting form
//   (14 KB/frame, HBM-bound) 59 us = 0.48 of 8 TB/s.  History: one frame per workgroup with everything re-fetched 121 us;
//   a 256-thread workgroup walking F frames with a five-pass radix-4 FFT (two block barriers per pass) 90 / 71 us --
//   7 us of barrier and LDS latency per frame and only five workgroups per CU to hide it.
//
// Inverse (vfx_istft): ONE kernel.  A workgroup owns IH = 16 hops of the overlap-add buffer (LDS) and runs the frames that
//   reach into them (IH + 4 = 20; IH = 2 for launches too small to fill the chip; the 4 halo frames are recomputed by the
//   neighbouring workgroup -- their spectra come from L2), one frame per wave at a time: Hermitian spectrum -> packed
//   1024-point complex inverse FFT (the same wave-level transform) -> x synthesis window -> added into the buffer.  Frames
//   that run together are at least five apart, so they touch disjoint samples, and a sample's contributions arrive in a fixed
//   order: five rounds, one block barrier each.  At the end every owned sample is divided by the window sum-of-squares
//   envelope (summed from the window on the fly) and written once.  The 16 KB-per-frame buffer of windowed frames that a
//   two-kernel form moves through HBM (write + read) does not exist.
//   torchlibrosa ISTFT semantics (see oracle/dsp.py): `y[:, n_fft//2 : n_fft//2 + length]`.
#include "stft_wave.h"

// (stft_wave.h turns floating-point contraction off and says why; repeated here so that this file does not depend on where a pragma
// of an included file ends)
#pragma clang fp contract(off)

namespace vfx {

// SPEC: the launch writes sp / cos / sin (any of them); false = the mel-only front-end of the restore path
template <bool SPEC>
__global__ __launch_bounds__(STFT_WAVES * 64, 2) void k_stft_mel(const float* __restrict__ wav, int L, int T,
                                                                 const float* __restrict__ window,
                                                                 const float2* __restrict__ tw,
                                                                 const float2* __restrict__ rtw,
                                                                 const float* __restrict__ fb_val,
                                                                 const int* __restrict__ fb_start,
                                                                 const int* __restrict__ fb_off, float* __restrict__ mel,
                                                                 float* __restrict__ sp, float* __restrict__ cosp,
                                                                 float* __restrict__ sinp, int log10_mel, int hop, float eps,
                                                                 int F, int groups, int total_groups, int fb_lds,
                                                                 const int* __restrict__ lens) {
  __shared__ float2 twl[NC];
  __shared__ float2 wl[NC];  // the window, as pairs (w[2n], w[2n+1])
  __shared__ float fbl[kMelNnzMax];  // the non-zeros of the mel filterbank (band-major): the band sums read them once per frame
  __shared__ float2 zbuf[STFT_WAVES][ZP];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int lane = tid & 63;
#pragma unroll
  for (int r = 0; r < NC / (STFT_WAVES * 64); ++r) {
    twl[tid + r * STFT_WAVES * 64] = tw[tid + r * STFT_WAVES * 64];
    wl[tid + r * STFT_WAVES * 64] = *reinterpret_cast<const float2*>(window + 2 * (tid + r * STFT_WAVES * 64));
  }
  if (mel && fb_lds)  // (a caller-supplied filterbank with more non-zeros than the table holds is read from global memory)
    for (int i = tid; i < fb_off[NMEL]; i += STFT_WAVES * 64) fbl[i] = fb_val[i];
  __syncthreads();  // the only block barrier: from here on the waves are independent
  const int gw = blockIdx.x * STFT_WAVES + wave;  // this wave's group of F consecutive frames of one clip
  if (gw >= total_groups) return;
  const int b = gw / groups, g = gw - b * groups;
  // `lens` (batches of clips of unequal length, vfx_restore_gsr_varlen): clip b holds lens[b] <= L samples in its row of L --
  // its frames, and the reflection at its end, are those of a clip of that length; the rows of the outputs past its
  // last frame are written as zeros (finite input for whatever reads the padded batch)
  const int Lrow = L;
  int Tc = T;  // frames of this clip (T stays the row stride of the outputs)
  if (lens) {
    L = lens[__builtin_amdgcn_readfirstlane(b)];
    Tc = min(T, L / hop + 1);
    const int t0 = g * F, t1 = min(T, t0 + F);
    for (int t = max(t0, Tc); t < t1; ++t) {
      const int64_t row = (int64_t)b * T + t;
      if (mel) {
        mel[row * NMEL + lane] = log10_mel ? -8.f : 0.f;
        mel[row * NMEL + 64 + lane] = log10_mel ? -8.f : 0.f;
      }
      if constexpr (SPEC)
        for (int k = lane; k < NBINS; k += 64) {
          if (sp) sp[row * NBINS + k] = 0.f;
          if (cosp) cosp[row * NBINS + k] = 0.f;
          if (sinp) sinp[row * NBINS + k] = 0.f;
        }
    }
    if (t0 >= Tc) return;
  }
  const int t_begin = g * F, t_end = min(Tc, t_begin + F);
  const float* x = wav + (int64_t)b * Lrow;
  float2* zw = zbuf[wave];
  float* ms = reinterpret_cast<float*>(zw);  // the magnitudes of the frame, over the FFT buffer once it is consumed

  // constants of the frame walk: this lane's two mel bands
  int f0[2], o0[2], nb[2];
  // (band lane and band 127 - lane: the bands grow with the frequency -- 1 .. 55 bins -- so every lane sums about 32 products)
  const int band[2] = {lane, NMEL - 1 - lane};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f0[h] = fb_start[band[h]];
    o0[h] = fb_off[band[h]];
    nb[h] = fb_off[band[h] + 1] - o0[h];
  }

  const float2 rtw_lane = rtw[lane];
  float2 xin[16];
  load_frame(x, L, t_begin, hop, lane, xin);
  for (int t = t_begin; t < t_end; ++t) {
    asm volatile("" : "+v"(lane));  // the frame-independent LDS addresses are recomputed per frame, not kept (and spilled)
    float2 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float2 ww = wl[lane + 64 * r];
      v[r] = make_float2(xin[r].x * ww.x, xin[r].y * ww.y);
    }
    if (t + 1 < t_end) load_frame(x, L, t + 1, hop, lane, xin);  // in flight during this frame's FFT
    wfft1024<-1>(v, zw, twl, lane);
    // the untangle pairs Z[k] with Z[1024 - k], which another lane holds; Z[1024] = Z[0] is lane 0's own v[0]
    float2 zn[16];
    mirror_bins(v, zn, zw, lane);  // zw is free: the magnitudes go over it
    if (lane == 0) zn[0] = v[0];
    __builtin_amdgcn_sched_barrier(0);

    const int64_t row = ((int64_t)b * T + t) * NBINS;
    auto bin = [&](int k, float2 zk, float2 znk, float2 wk) __attribute__((always_inline)) {
      float re, im, mag;
      untangle_bin(zk, znk, wk, eps, re, im, mag);
      ms[k] = mag;
      if constexpr (!SPEC) return;
      if (sp) sp[row + k] = mag;
      if (cosp || sinp) {
        const float inv = __builtin_amdgcn_rcpf(mag);  // v_rcp_f32 (1 ulp); mag = 0 (eps = 0, silent bin): inf, 0 * inf = NaN like 0 / 0
        if (cosp) cosp[row + k] = re * inv;
        if (sinp) sinp[row + k] = im * inv;
      }
    };
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      bin(lane + 64 * m, v[m], zn[m], rtw_of(rtw_lane, m));
      if ((m & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four bins at a time: their temporaries are not 16-fold live
    }
    if (lane == 0) bin(NC, v[0], zn[0], make_float2(-1.f, 0.f));  // Z[1024] = Z[0], W^1024 = -1
    wave_sync();
    if (mel) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // four chains (the loads of the loop do not depend on the sums)
        const float* mp = ms + f0[h];
        auto band_sum = [&](auto fp) __attribute__((always_inline)) {
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
          int i = 0;
          for (; i + 3 < nb[h]; i += 4) {
            a0 = fmaf(mp[i], fp[i], a0);
            a1 = fmaf(mp[i + 1], fp[i + 1], a1);
            a2 = fmaf(mp[i + 2], fp[i + 2], a2);
            a3 = fmaf(mp[i + 3], fp[i + 3], a3);
          }
          for (; i < nb[h]; ++i) a0 = fmaf(mp[i], fp[i], a0);
          return (a0 + a2) + (a1 + a3);
        };
        const float acc = fb_lds ? band_sum(fbl + o0[h]) : band_sum(fb_val + o0[h]);
        mel[((int64_t)b * T + t) * NMEL + band[h]] = log10_mel ? log10f(fmaxf(acc, 1e-8f)) : acc;
      }
    }
    wave_sync();  // ms is consumed before the next frame's first pass writes the buffer
  }
}

__global__ __launch_bounds__(128) void k_mel_project(const float* __restrict__ sp, int64_t rows,
                                                      const float* __restrict__ fb_val,
                                                      const int* __restrict__ fb_start,
                                                      const int* __restrict__ fb_off, float* __restrict__ mel) {
  __shared__ float s[NBINS + 3];
  const int64_t row = blockIdx.x;
  for (int k = threadIdx.x; k < NBINS; k += 128) s[k] = sp[row * NBINS + k];
  __syncthreads();
  const int j = threadIdx.x;
  const int f0 = fb_start[j], o0 = fb_off[j], n = fb_off[j + 1] - o0;
  float acc = 0.f;
  for (int i = 0; i < n; ++i) acc = fmaf(s[f0 + i], fb_val[o0 + i], acc);
  mel[row * NMEL + j] = acc;
}

// Inverse.  Per frame: x[n] (n < 2048) = irfft(X)[n] * window[n]:
//   pack Z[k] = E[k] + i O[k] with E = (X[k] + conj X[N-k]) / 2, O = conj(W^k) (X[k] - conj X[N-k]) / 2;
//   z = IFFT1024(Z) / 1024;  x[2n] = Re z[n], x[2n+1] = Im z[n].
// Overlap-add: wav[b, n] = (sum_t x_t[p - t*hop]) / (sum_t window[p - t*hop]^2), p = n + 1024, for every n < L inside the
// overlap-add buffer (p < 2048 + hop*(T-1)); 0 beyond it.  This is torchlibrosa's `y[:, n_fft//2 : n_fft//2 + length]`
// (same in the in-repo twin tools/dsp/base.py:193-200, `end = start + length`): the L mod hop samples past hop*(T-1) are
// reconstructed from the tails of the last frames.  Positions whose envelope is tiny are left undivided
// (librosa.filters.window_sumsquare semantics).
// A workgroup owns IH hops of the overlap-add buffer (LDS) and runs the frames that reach into them, four at a time: each
// wave packs and inverse-transforms its own frame (wave-level FFT, no barrier) and adds it into the buffer; which frames run
// together is chosen so that they cannot touch the same sample (see the kernel).
// IH = 16 (20 frames per workgroup) for large launches, 2 (6 frames, three times the inverse FFTs but a fraction of the serial
// chain) when there are too few frames to fill the chip (streaming chunks).
//
// Low-pass by STFT masking (vfx_stft_lowpass, k_stft_lowpass): the SAME workgroup, with the spectrum of a frame made on the
// spot instead of read -- the wave that owns the frame loads its samples (the forward kernel's load_frame, the clip's own
// reflection), windows and transforms them, untangles the bins exactly as k_stft_mel does, forms mag, cos = re / mag,
// sin = im / mag and X = (mag cos, mag sin), zero from the clip's cut-off bin up, and hands X[k] / X[1024 - k] to the pack
// above.  No spectrum in HBM; the 4 halo frames of a group are transformed forward by both neighbours ((IH + 4) / IH forward
// FFTs per frame).  Every expression is the one the two-launch path (k_stft_mel<true>, sp * cos and sp * sin by torch, k_istft)
// evaluates, so the samples are bit for bit that path's.
//
// Splice (vfx_stft_splice, k_stft_splice): the same workgroup once more, over TWO rows -- the input x and the restored clip y.  The
// wave loads the frame from both, forms d = x - g y in registers, makes the spectrum of d as above with the weight a[k] of splice.py's
// ramp_weights in place of the hard mask, and the final loop adds g y back: g y + ISTFT(a . STFT(x - g y)), which by linearity is
// ISTFT(a STFT(x) + (1 - a) STFT(g y)) -- x below the seam, g y above -- with one forward transform per frame.  Bit for bit the chain
// torch (g y, x - g y), k_stft_mel<true>, torch (the products and weights), k_istft, torch (+).

// a * b rounded to float32 ON ITS OWN: never the multiplication of an FMA.  The two-launch path stores mag * cos and mag * sin
// to memory as float32 before the pack adds them; here the products feed straight into the pack's sums.  (The file's pragma says
// so already; this one keeps the fence where it is needed whatever happens to that one.)
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// One frame of the low-pass, by the wave that owns it.  In: xk = the sixteen sample pairs load_frame left.  Out: xk[r] = X[k],
// xn[r] = X[1024 - k], k = lane + 64 r -- what k_istft's load_spectrum leaves -- with X = 0 for the bins k >= cut.
// RAMP (k_stft_splice): the bins cut - ramp <= k < cut are weighted by a[k] = float(cut - k) / float(ramp + 1) -- one division, computed
// from k, no table -- each of the two products times a[k], rounded on its own; the bins below them (a = 1) are left as they are.
// ramp = 0 is the hard mask.
template <bool RAMP>
__device__ __forceinline__ void lowpass_spectrum(float2 (&xk)[16], float2 (&xn)[16], float2* zw, const float2* twl,
                                                 const float2* wl, float2 rtw_lane, int lane, int cut, int ramp) {
  asm volatile("" : "+v"(rtw_lane.x), "+v"(rtw_lane.y));  // the sixteen W^k are made per frame, not kept across the frame walk (and spilled)
  float2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float2 ww = wl[lane + 64 * r];
    v[r] = make_float2(xk[r].x * ww.x, xk[r].y * ww.y);
  }
  wfft1024<-1>(v, zw, twl, lane);
  mirror_bins(v, xn, zw, lane);
  if (lane == 0) xn[0] = v[0];  // Z[1024] = Z[0]
  __builtin_amdgcn_sched_barrier(0);
  auto bin = [&](int k, float2 zk, float2 znk, float2 wk) __attribute__((always_inline)) {
    float re, im, mag;
    untangle_bin(zk, znk, wk, 1e-8f, re, im, mag);  // eps of wav_to_spectrogram_phase
    const float inv = __builtin_amdgcn_rcpf(mag);
    const float c = re * inv, s = im * inv;  // what k_stft_mel stores as cos / sin
    if constexpr (RAMP) {
      float2 X = make_float2(mul_rounded(mag, c), mul_rounded(mag, s));
      if (k >= cut - ramp) {
        const float a = __fdiv_rn((float)(cut - k), (float)(ramp + 1));
        X = make_float2(mul_rounded(X.x, a), mul_rounded(X.y, a));
      }
      return k >= cut ? make_float2(0.f, 0.f) : X;
    } else {  // (the low-pass's own expression, kept as it was: k_stft_lowpass compiles to the instructions it had)
      return k >= cut ? make_float2(0.f, 0.f) : make_float2(mul_rounded(mag, c), mul_rounded(mag, s));
    }
  };
  float2 top = make_float2(0.f, 0.f);
  if (lane == 0) top = bin(NC, v[0], xn[0], make_float2(-1.f, 0.f));  // Z[1024] = Z[0], W^1024 = -1
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    xk[m] = bin(lane + 64 * m, v[m], xn[m], rtw_of(rtw_lane, m));
    if ((m & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // four bins at a time, as in the forward kernel
  }
  if (lane == 0) zw[ZP - 1] = top;  // X[1024]: the partner of k = 0
  mirror_bins(xk, xn, zw, lane);
}

// Where a workgroup of the inverse takes its spectrum from
enum IstftMode {
  ISTFT_SPECTRUM,  // k_istft: re / im (B, T, 1025)
  ISTFT_LOWPASS,   // k_stft_lowpass: made from the rows of `src` (B, L) as above, masked from bin cuts[b] up; re / im are not read
  ISTFT_SPLICE     // k_stft_splice: made from d = src - gains[b] * src2 (both (B, L)) with the ramp below cuts[b], and gains[b] * src2
                   // is added to the samples at the end
};

// One workgroup of the inverse.
template <IstftMode MODE>
__device__ __forceinline__ void istft_group(const float* __restrict__ re, const float* __restrict__ im,
                                            const float* __restrict__ src, const float* __restrict__ src2,
                                            const int* __restrict__ cuts, const int* __restrict__ gains, int ramp,
                                            const float* __restrict__ window, const float2* __restrict__ tw,
                                            const float2* __restrict__ rtw, int T, int L, int hop, int groups, int IH,
                                            float* __restrict__ wav, const int* __restrict__ lens) {
  __shared__ float2 twl[NC];
  __shared__ float2 wl[NC];  // the synthesis window, as pairs (ISTFT_LOWPASS, ISTFT_SPLICE: the analysis window too)
  __shared__ float2 zbuf[STFT_WAVES][ZP];
  extern __shared__ __attribute__((aligned(16))) float ola[];  // [IH * hop]
  const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int lane = tid & 63;
  const int span = IH * hop;
  const int p0 = g * span;                      // first owned position of the un-trimmed overlap-add buffer
  // `lens` (a batch of clips of unequal length): clip b has lens[b] <= L samples, i.e. Tc = lens[b] / hop + 1 <= T frames -- the
  // later frames of its rows of re / im do not exist for it and its samples past lens[b] are written as zeros; T and L stay the
  // row strides
  const int Ts = T, Ls = L;
  if (lens) {
    L = lens[b];
    T = min(T, L / hop + 1);
  }
  const int t_lo = max(0, g * IH - (NFFT - 1) / hop), t_hi = min(T - 1, g * IH + IH - 1);
  for (int i = tid; i < span; i += STFT_WAVES * 64) ola[i] = 0.f;
#pragma unroll
  for (int r = 0; r < NC / (STFT_WAVES * 64); ++r) {
    twl[tid + r * STFT_WAVES * 64] = tw[tid + r * STFT_WAVES * 64];
    wl[tid + r * STFT_WAVES * 64] = *reinterpret_cast<const float2*>(window + 2 * (tid + r * STFT_WAVES * 64));
  }
  const float sc = 1.0f / NC;
  const float2 rtw_lane = rtw[lane];
  __syncthreads();  // ola zeroed, twl and wl complete

  // the spectrum of this wave's frame of a round: (Re, Im) of bins k and 1024 - k, k = lane + 64 r
  // (ISTFT_LOWPASS: what is requested ahead is the frame's samples, in xk; lowpass_spectrum turns them into the spectrum in place.
  // ISTFT_SPLICE: the samples of both rows, the second in yk, at the same indices)
  float2 xk[16], xn[16];
  [[maybe_unused]] float2 yk[16];
  [[maybe_unused]] float gain = 1.f;
  if constexpr (MODE == ISTFT_SPLICE) gain = __int_as_float(gains[b]);  // (a float32 bit pattern: the host arrays travel in int rows)
  auto load_spectrum = [&](int t) __attribute__((always_inline)) {
    if constexpr (MODE == ISTFT_SPLICE) {
      load_frame(src + (int64_t)b * Ls, L, t, hop, lane, xk);
      load_frame(src2 + (int64_t)b * Ls, L, t, hop, lane, yk);
    } else if constexpr (MODE == ISTFT_LOWPASS) {
      load_frame(src + (int64_t)b * Ls, L, t, hop, lane, xk);
    } else {
      const float* R = re + ((int64_t)b * Ts + t) * NBINS;
      const float* I = im + ((int64_t)b * Ts + t) * NBINS;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned k = (unsigned)(lane + 64 * r);
        xk[r] = make_float2(ldg32(R, k), ldg32(I, k));
        xn[r] = make_float2(ldg32(R, NC - k), ldg32(I, NC - k));
      }
    }
  };
  // Frames at least D apart touch disjoint samples.  Round r (D rounds, one block barrier each) takes the frames t = r (mod D)
  // -- the ABSOLUTE frame index -- of the workgroup's n frames, wave w every fourth of them: the frames of a round add into the
  // buffer CONCURRENTLY and never meet, and a sample's contributions arrive in the order of t mod D -- sums that depend neither
  // on timing nor on how the buffer is cut into groups (IH, which the launch picks from the batch size): a clip's samples are
  // bit-identical whatever batch it is restored in.
  const int D = (NFFT + hop - 1) / hop;
  const int n = t_hi - t_lo + 1;
  // this wave's frame list in processing order: (r, f) with f = ((r - t_lo) mod D) + D (wave + 4 j), f = t - t_lo
  auto first_in_round = [&](int r) __attribute__((always_inline)) { return ((r - t_lo) % D + D) % D + D * wave; };
  int r = 0, f = first_in_round(0);
  while (r < D && f >= n) f = first_in_round(++r);  // the first frame of this wave, if any
  if (r < D) load_spectrum(t_lo + f);
  for (int round = 0; round < D; ++round) {  // block-uniform trip count
    while (r == round) {
      const int t = t_lo + f;
      asm volatile("" : "+v"(lane));  // as in the forward kernel
      if constexpr (MODE == ISTFT_SPLICE) {
#pragma unroll
        for (int q = 0; q < 16; ++q)  // d = x - g y: the product rounded, then one subtraction
          xk[q] = make_float2(xk[q].x - mul_rounded(gain, yk[q].x), xk[q].y - mul_rounded(gain, yk[q].y));
        lowpass_spectrum<true>(xk, xn, zbuf[wave], twl, wl, rtw_lane, lane, cuts[b], ramp);
      }
      if constexpr (MODE == ISTFT_LOWPASS) lowpass_spectrum<false>(xk, xn, zbuf[wave], twl, wl, rtw_lane, lane, cuts[b], 0);
      float2 v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float2 d = make_float2(0.5f * (xk[q].x - xn[q].x), 0.5f * (xk[q].y + xn[q].y));
        float2 wk = rtw_of(rtw_lane, q);
        wk.y = -wk.y;  // conj(W^k) = e^{+2 pi i k / 2048}
        const float2 o = cmul(wk, d);
        v[q] = make_float2(fmaf(0.5f, xk[q].x + xn[q].x, -o.y), fmaf(0.5f, xk[q].y - xn[q].y, o.x));  // Z = E + i O
      }
      // advance to this wave's next frame and request its spectrum: it travels during this frame's FFT
      f += D * STFT_WAVES;
      while (r < D && f >= n) f = first_in_round(++r);
      if (r < D) load_spectrum(t_lo + f);
      wfft1024<1>(v, zbuf[wave], twl, lane);
      const int off = t * hop - p0;  // frame sample o lands at owned index off + o
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const int i0 = off + 2 * (lane + 64 * m);
        const float2 ww = wl[lane + 64 * m];
        if (i0 >= 0 && i0 < span) ola[i0] = fmaf(v[m].x * sc, ww.x, ola[i0]);  // one lane per sample, no other frame of the round nearby
        if (i0 + 1 >= 0 && i0 + 1 < span) ola[i0 + 1] = fmaf(v[m].y * sc, ww.y, ola[i0 + 1]);
      }
    }
    __syncthreads();
  }
  const int total = NFFT + hop * (T - 1);
  for (int i = tid; i < span; i += STFT_WAVES * 64) {
    const int p = p0 + i, n = p - NFFT / 2;
    if (n < 0 || n >= Ls) continue;
    float out = 0.f;
    if (p < total && n < L) {
      float env = 0.f;
      int th = p / hop;                        // last frame starting at or before p
      if (th > T - 1) th = T - 1;
      int tl = (p - NFFT + hop) / hop;         // first frame with t*hop + 2048 > p
      if (tl < 0) tl = 0;
      for (int t = tl; t <= th; ++t) {
        const int o = p - t * hop;
        if (o >= 0 && o < NFFT) {
          const float ww = window[o];
          env = fmaf(ww, ww, env);
        }
      }
      out = env > 1.1754944e-38f ? ola[i] / env : ola[i];
      if constexpr (MODE == ISTFT_SPLICE) out = mul_rounded(gain, src2[(int64_t)b * Ls + n]) + out;  // g y, the same rounded product, + r
    }
    wav[(int64_t)b * Ls + n] = out;
  }
}

__global__ __launch_bounds__(STFT_WAVES * 64, 2) void k_istft(const float* __restrict__ re, const float* __restrict__ im,
                                                              const float* __restrict__ window, const float2* __restrict__ tw,
                                                              const float2* __restrict__ rtw, int T, int L, int hop, int groups,
                                                              int IH, float* __restrict__ wav, const int* __restrict__ lens) {
  istft_group<ISTFT_SPECTRUM>(re, im, nullptr, nullptr, nullptr, nullptr, 0, window, tw, rtw, T, L, hop, groups, IH, wav, lens);
}

// wav (B, L), clip b = its first lens[b] samples (1024 < lens[b] <= L) -> out (B, L): the clip with the STFT bins from cut[b] up
// removed, zeros past lens[b].  `window` is both the analysis and the synthesis window.  `out` must not overlap `wav`: a workgroup
// reads samples its neighbours own.
__global__ __launch_bounds__(STFT_WAVES * 64, 2) void k_stft_lowpass(const float* __restrict__ wav, const int* __restrict__ lens,
                                                                     const int* __restrict__ cut,
                                                                     const float* __restrict__ window,
                                                                     const float2* __restrict__ tw,
                                                                     const float2* __restrict__ rtw, int T, int L, int hop,
                                                                     int groups, int IH, float* __restrict__ out) {
  istft_group<ISTFT_LOWPASS>(nullptr, nullptr, wav, nullptr, cut, nullptr, 0, window, tw, rtw, T, L, hop, groups, IH, out, lens);
}

// x, y (B, L), pair b = the first lens[b] samples of both rows (1024 < lens[b] <= L) -> out (B, L) = g y + ISTFT(a . STFT(x - g y)),
// g = gains[b] (a float32 bit pattern), a = 1 below bin cut[b] - ramp, 0 from cut[b] up, the linear ramp between; zeros past lens[b].
// By linearity ISTFT(a STFT(x) + (1 - a) STFT(g y)): x below the seam, g y above it, with one forward transform per frame.  `out` must
// overlap neither x nor y; nothing at or past lens[b] of either row is read.
__global__ __launch_bounds__(STFT_WAVES * 64, 2) void k_stft_splice(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const int* __restrict__ lens, const int* __restrict__ cut,
                                                                    const int* __restrict__ gains, int ramp,
                                                                    const float* __restrict__ window, const float2* __restrict__ tw,
                                                                    const float2* __restrict__ rtw, int T, int L, int hop, int groups,
                                                                    int IH, float* __restrict__ out) {
  istft_group<ISTFT_SPLICE>(nullptr, nullptr, x, y, cut, gains, ramp, window, tw, rtw, T, L, hop, groups, IH, out, lens);
}

// Frames per wave of the forward kernel: as many as keep the launch at about one round of resident waves
// (2 workgroups of 4 waves per CU -- 59 KB of LDS -- x 256 CUs), at most 32.
int frames_per_group(int64_t frames) {
  const int64_t f = (frames + 2047) / 2048;
  return (int)std::max<int64_t>(1, std::min<int64_t>(32, f));
}

void launch_stft_mel(const FrontEndTables& t, const float* wav, int B, int L, int T, float* mel, float* sp,
                     float* cosp, float* sinp, int log10_mel, int hop, float eps, hipStream_t stream, const int* lens) {
  const int F = frames_per_group((int64_t)B * T);
  const int groups = (T + F - 1) / F;
  const int total = B * groups;
  auto kernel = (sp || cosp || sinp) ? k_stft_mel<true> : k_stft_mel<false>;
  hipLaunchKernelGGL(kernel, dim3((total + STFT_WAVES - 1) / STFT_WAVES), dim3(STFT_WAVES * 64), 0, stream, wav, L, T, t.window,
                     reinterpret_cast<const float2*>(t.twiddle), reinterpret_cast<const float2*>(t.rtwiddle),
                     t.fb_val, t.fb_start, t.fb_off, mel, sp, cosp, sinp, log10_mel, hop, eps, F, groups, total,
                     t.fb_nnz <= kMelNnzMax ? 1 : 0, lens);
  VFX_HIP(hipGetLastError());
}

void launch_mel_project(const FrontEndTables& t, const float* sp, int64_t rows, float* mel, hipStream_t stream) {
  hipLaunchKernelGGL(k_mel_project, dim3((unsigned)rows), dim3(128), 0, stream, sp, rows, t.fb_val, t.fb_start,
                     t.fb_off, mel);
  VFX_HIP(hipGetLastError());
}

// The inverse's launch geometry: IH hops per workgroup, and the groups that cover the positions [0, 1024 + L) of the un-trimmed
// overlap-add buffer
IstftGrid istft_grid(int B, int T, int L, int hop) {
  IstftGrid g;
  g.IH = (int64_t)B * T >= 4096 ? 16 : 2;
  g.span = g.IH * hop;
  g.groups = (NFFT / 2 + L + g.span - 1) / g.span;
  return g;
}

void launch_istft(const FrontEndTables& t, const float* re, const float* im, int B, int T, int L, int hop, float* wav,
                  hipStream_t stream, const int* lens) {
  const IstftGrid g = istft_grid(B, T, L, hop);
  hipLaunchKernelGGL(k_istft, dim3(B * g.groups), dim3(256), (size_t)g.span * sizeof(float), stream, re, im, t.window,
                     reinterpret_cast<const float2*>(t.twiddle), reinterpret_cast<const float2*>(t.rtwiddle), T, L, hop,
                     g.groups, g.IH, wav, lens);
  VFX_HIP(hipGetLastError());
}

void launch_stft_lowpass(const FrontEndTables& t, const float* wav, int B, int L, int hop, const int* lens, const int* cut,
                         float* out, hipStream_t stream) {
  const int T = L / hop + 1;  // frames of a clip that fills its row
  const IstftGrid g = istft_grid(B, T, L, hop);
  hipLaunchKernelGGL(k_stft_lowpass, dim3(B * g.groups), dim3(256), (size_t)g.span * sizeof(float), stream, wav, lens, cut,
                     t.window, reinterpret_cast<const float2*>(t.twiddle), reinterpret_cast<const float2*>(t.rtwiddle), T, L,
                     hop, g.groups, g.IH, out);
  VFX_HIP(hipGetLastError());
}

void launch_stft_splice(const FrontEndTables& t, const float* x, const float* y, int B, int L, int hop, const int* lens, const int* cut,
                        const int* gains, int ramp, float* out, hipStream_t stream) {
  const int T = L / hop + 1;  // frames of a clip that fills its row
  const IstftGrid g = istft_grid(B, T, L, hop);
  hipLaunchKernelGGL(k_stft_splice, dim3(B * g.groups), dim3(256), (size_t)g.span * sizeof(float), stream, x, y, lens, cut, gains, ramp,
                     t.window, reinterpret_cast<const float2*>(t.twiddle), reinterpret_cast<const float2*>(t.rtwiddle), T, L, hop,
                     g.groups, g.IH, out);
  VFX_HIP(hipGetLastError());
}

}  // namespace vfx
