// mix.hip -- noise mixed into batches of float32 clips at a given SNR weight and scale: the device form of add_noise_and_scale,
// add_noise_and_scale_with_HQ and add_noise_and_scale_with_HQ_with_Aug (dataloaders/augmentation/base.py:33-118, mirrored in
// simulate.py).  form 0 = plain (front, noise), 1 = with HQ (hq, front, noise), 2 = with HQ and Aug (hq, front, aug, noise); the
// "speech" the noise is mixed into is front in forms 0 and 1 and aug in form 2.
//
// Per clip, in the host code's order (every elementwise step is ONE IEEE float32 operation per sample, every per-clip scalar is
// computed in double from float32 peaks / float64 sums and rounded to float32 once -- NumPy's arithmetic on a float32 array with a
// Python-float operand; contraction is off for the whole file):
//   1. peaks      p_x = max |x| of every input over the clip's own samples
//   2. normalise  noise / p_noise;  form 0: front / p_front;  forms 1, 2: hq, front (, aug) * float(1.0 / max of their peaks)
//   3. level      forms 1, 2: level = mean |speech|; if level > 0.02: noise / float(mean |noise| / level)
//   4. SNR        noise / float(w), when weights are given
//   5. peak 2     max |.| over noise + speech and every returned signal; all of them * float(1.0 / peak)
//   6. scale      all of them * float(scale)
//   7. noisy      noise_out + speech_out
//
// Passes over memory (each one grid over the batch: blockIdx.y = clip, blockIdx.x = chunk of kClipChunk samples of it):
//   k_mix_peaks    reads every input                     -> p_x (atomicMax on the bit pattern of |x|)
//   k_mix_sums     forms 1, 2: reads speech, noise        -> per-chunk float64 sums of |speech * s1| and |noise / p_noise|
//   k_mix_level    forms 1, 2: one wave per clip          -> the chunk sums added in index order, the level rule, float(ratio)
//   k_mix_mixpeak  reads speech, noise                    -> max |noise2 + speech1|
//   k_mix_apply    reads what it returns, writes it       -> outputs, rows zero from the clip's length up to ld
// The peaks of the merely rescaled signals need no pass: rounding is monotonic, max |fl(x * s)| = fl(max |x| * s) (and the same for a
// division by a positive scalar), so steps 2-4 applied to p_x give them.  "max" over several signals is Python's max() over floats
// in the host's argument order (a later value replaces the current one only when it compares greater), NaN behaviour included.
//
// The sample groups of a thread and the peak commit are clip_batch.h's; the float64 sums of a chunk add the same samples in the same
// order whatever the row's address (simulate pads the stride of its batches to a multiple of 4, which keeps every row on the fast path).
#include "clip_batch.h"
#include "vfx_internal.h"

#pragma clang fp contract(off)

namespace vfx {

constexpr int kMixThreads = 256;
constexpr int kMixGroups = kClipChunk / (4 * kMixThreads);  // groups of 4 samples per thread
static_assert(kClipChunk == 4 * kMixThreads * kMixGroups, "a chunk is whole groups of every thread");
enum { MIX_FRONT = 0, MIX_NOISE = 1, MIX_HQ = 2, MIX_AUG = 3, MIX_MIXTURE = 4 };  // rows of in / out / a clip's peaks

struct MixLevel {
  float ratio;  // float(mean |noise| / mean |speech|)
  int match;    // the level rule applies: noise / ratio
};

struct MixArgs {
  const float* in[4];  // front, noise, hq, aug: (clips, ld), NULL where the form has none
  float* out[5];       // front, noise, hq, aug, noisy: (clips, ld), NULL where not wanted
  unsigned* peaks;     // (clips, kMixPeaks) bit patterns of max |.|: the inputs and the mixture, zeroed before the launches
  double* partial;     // (clips, nchunk, 2) chunk sums of |speech1|, |noise1|
  MixLevel* level;     // (clips)
  int64_t ld;
  int form, has_w, nchunk;
  int len[kMixMaxClips];
  float w[kMixMaxClips], scale[kMixMaxClips];  // float(10 ** (snr / 20)), float(scale)
};

__device__ __forceinline__ float mix_pymax(float cur, float nxt) { return nxt > cur ? nxt : cur; }  // one step of Python's max()

// steps 2-4 as they apply to one sample (or to a peak)
struct MixScalars {
  float p_noise;  // noise / p_noise
  float s1;       // form 0: front / s1;  forms 1, 2: hq, front, aug * s1
  float ratio, w;
  bool match, has_w, form0;
  __device__ __forceinline__ float speech(float x) const { return form0 ? x / s1 : x * s1; }
  __device__ __forceinline__ float noise(float x) const {
    float v = x / p_noise;
    if (match) v = v / ratio;
    if (has_w) v = v / w;
    return v;
  }
};

__device__ __forceinline__ MixScalars mix_scalars(const MixArgs& a, int b, bool with_level) {
  const unsigned* pk = a.peaks + b * kMixPeaks;
  MixScalars s;
  s.form0 = a.form == 0;
  s.p_noise = __uint_as_float(pk[MIX_NOISE]);
  if (s.form0) {
    s.s1 = __uint_as_float(pk[MIX_FRONT]);
  } else {  // unify_energy(HQ, front[, augfront])
    float m = mix_pymax(__uint_as_float(pk[MIX_HQ]), __uint_as_float(pk[MIX_FRONT]));
    if (a.form == 2) m = mix_pymax(m, __uint_as_float(pk[MIX_AUG]));
    s.s1 = (float)(1.0 / (double)m);
  }
  s.match = false;
  s.ratio = 1.f;
  if (with_level && !s.form0) {
    const MixLevel l = a.level[b];
    s.match = l.match != 0;
    s.ratio = l.ratio;
  }
  s.has_w = a.has_w != 0;
  s.w = a.w[b];
  return s;
}

__global__ __launch_bounds__(kMixThreads) void k_mix_peaks(const MixArgs a) {
  const int b = blockIdx.y;
  const int64_t n = a.len[b], c0 = (int64_t)blockIdx.x * kClipChunk;
  if (c0 >= n) return;
  __shared__ unsigned wave_peak[4][kMixThreads / 64];  // a set per signal: no barrier between the commits
#pragma unroll
  for (int sig = 0; sig < 4; ++sig) {
    if (!a.in[sig]) continue;  // (the same for every thread of the workgroup, as the return above)
    const float* row = a.in[sig] + (int64_t)b * a.ld;
    const bool vec = clip_aligned(row);
    float v[kMixGroups][4];
#pragma unroll
    for (int k = 0; k < kMixGroups; ++k) clip_load(row, vec, c0 + 4 * (threadIdx.x + kMixThreads * k), n, v[k]);
    unsigned peak = 0;  // (a sample past n was loaded as +0: bit pattern 0)
#pragma unroll
    for (int k = 0; k < kMixGroups; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) peak = max(peak, ClipType<float>::abs_bits(v[k][e]));
    clip_commit_peak<kMixThreads>(peak, a.peaks + b * kMixPeaks + sig, wave_peak[sig]);
  }
}

__global__ __launch_bounds__(kMixThreads) void k_mix_sums(const MixArgs a) {
  __shared__ double wsum[kMixThreads / 64][2];
  const int b = blockIdx.y;
  const int64_t n = a.len[b], c0 = (int64_t)blockIdx.x * kClipChunk;
  if (c0 >= n) return;
  const MixScalars sc = mix_scalars(a, b, false);
  const float* sp = a.in[a.form == 2 ? MIX_AUG : MIX_FRONT] + (int64_t)b * a.ld;
  const float* ns = a.in[MIX_NOISE] + (int64_t)b * a.ld;
  const bool vsp = clip_aligned(sp), vns = clip_aligned(ns);
  float x[kMixGroups][4], z[kMixGroups][4];
#pragma unroll
  for (int k = 0; k < kMixGroups; ++k) {
    const int64_t j = c0 + 4 * (threadIdx.x + kMixThreads * k);
    clip_load(sp, vsp, j, n, x[k]);
    clip_load(ns, vns, j, n, z[k]);
  }
  double s_sp = 0.0, s_ns = 0.0;  // the thread's samples in index order
#pragma unroll
  for (int k = 0; k < kMixGroups; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + 4 * (threadIdx.x + kMixThreads * k) + e < n) {
        s_sp += (double)fabsf(x[k][e] * sc.s1);
        s_ns += (double)fabsf(z[k][e] / sc.p_noise);
      }
  // a fixed butterfly over the wave, the waves in order: the chunk's sum depends on the chunk's samples alone
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s_sp += __shfl_xor(s_sp, d);
    s_ns += __shfl_xor(s_ns, d);
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][0] = s_sp, wsum[threadIdx.x >> 6][1] = s_ns;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t_sp = wsum[0][0], t_ns = wsum[0][1];
#pragma unroll
    for (int w = 1; w < kMixThreads / 64; ++w) t_sp += wsum[w][0], t_ns += wsum[w][1];
    double* dst = a.partial + ((int64_t)b * a.nchunk + blockIdx.x) * 2;
    dst[0] = t_sp;
    dst[1] = t_ns;
  }
}

// one wave per clip: the chunk sums in index order (loaded 64 at a time, added by lane 0), then _match_noise_level's rule
__global__ __launch_bounds__(64) void k_mix_level(const MixArgs a) {
  __shared__ double tile[64][2];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t n = a.len[b];
  const int nch = (int)((n + kClipChunk - 1) / kClipChunk);
  const double* src = a.partial + (int64_t)b * a.nchunk * 2;
  double t_sp = 0.0, t_ns = 0.0;
  for (int c0 = 0; c0 < nch; c0 += 64) {
    const int m = min(64, nch - c0);
    __syncthreads();
    if (lane < m) tile[lane][0] = src[(c0 + lane) * 2], tile[lane][1] = src[(c0 + lane) * 2 + 1];
    __syncthreads();
    if (lane == 0)
      for (int i = 0; i < m; ++i) t_sp += tile[i][0], t_ns += tile[i][1];
  }
  if (lane == 0) {
    const double level = t_sp / (double)n;
    MixLevel l{1.f, 0};
    if (level > 0.02) {
      l.ratio = (float)((t_ns / (double)n) / level);
      l.match = 1;
    }
    a.level[b] = l;
  }
}

__global__ __launch_bounds__(kMixThreads) void k_mix_mixpeak(const MixArgs a) {
  const int b = blockIdx.y;
  const int64_t n = a.len[b], c0 = (int64_t)blockIdx.x * kClipChunk;
  if (c0 >= n) return;
  const MixScalars sc = mix_scalars(a, b, true);
  const float* sp = a.in[a.form == 2 ? MIX_AUG : MIX_FRONT] + (int64_t)b * a.ld;
  const float* ns = a.in[MIX_NOISE] + (int64_t)b * a.ld;
  const bool vsp = clip_aligned(sp), vns = clip_aligned(ns);
  float x[kMixGroups][4], z[kMixGroups][4];
#pragma unroll
  for (int k = 0; k < kMixGroups; ++k) {
    const int64_t j = c0 + 4 * (threadIdx.x + kMixThreads * k);
    clip_load(sp, vsp, j, n, x[k]);
    clip_load(ns, vns, j, n, z[k]);
  }
  unsigned peak = 0;
#pragma unroll
  for (int k = 0; k < kMixGroups; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + 4 * (threadIdx.x + kMixThreads * k) + e < n) peak = max(peak, ClipType<float>::abs_bits(sc.noise(z[k][e]) + sc.speech(x[k][e])));
  __shared__ unsigned wave_peak[kMixThreads / 64];
  clip_commit_peak<kMixThreads>(peak, a.peaks + b * kMixPeaks + MIX_MIXTURE, wave_peak);
}

// float(1.0 / activelev(noise + speech, <the returned signals in the host's order>)): the mixture's peak from k_mix_mixpeak, the
// others from the inputs' peaks taken through steps 2-4
__device__ __forceinline__ float mix_second_scale(const MixArgs& a, int b, const MixScalars& sc) {
  const unsigned* pk = a.peaks + b * kMixPeaks;
  const float p_mix = __uint_as_float(pk[MIX_MIXTURE]);
  const float p_noise = sc.noise(__uint_as_float(pk[MIX_NOISE]));
  const float p_front = sc.speech(__uint_as_float(pk[MIX_FRONT]));
  float peak;
  if (a.form == 0) {  // unify_energy(noise + front, noise, front)
    peak = mix_pymax(mix_pymax(p_mix, p_noise), p_front);
  } else {
    const float p_hq = sc.speech(__uint_as_float(pk[MIX_HQ]));
    if (a.form == 1) {  // unify_energy(noise + front, noise, front, HQ)
      peak = mix_pymax(mix_pymax(mix_pymax(p_mix, p_noise), p_front), p_hq);
    } else {  // unify_energy(noise + augfront, augfront, noise, front, HQ)
      const float p_aug = sc.speech(__uint_as_float(pk[MIX_AUG]));
      peak = mix_pymax(mix_pymax(mix_pymax(mix_pymax(p_mix, p_aug), p_noise), p_front), p_hq);
    }
  }
  return (float)(1.0 / (double)peak);
}

__global__ __launch_bounds__(kMixThreads) void k_mix_apply(const MixArgs a) {
  const int b = blockIdx.y;
  const int64_t n = a.len[b], c0 = (int64_t)blockIdx.x * kClipChunk;
  if (c0 >= a.ld) return;
  const MixScalars sc = mix_scalars(a, b, true);
  const float s2 = mix_second_scale(a, b, sc), scale = a.scale[b];
  const int speech_sig = a.form == 2 ? MIX_AUG : MIX_FRONT;
  const int64_t row0 = (int64_t)b * a.ld;
  bool vin[4], vout[5];
#pragma unroll
  for (int sig = 0; sig < 4; ++sig) vin[sig] = a.in[sig] && clip_aligned(a.in[sig] + row0);
#pragma unroll
  for (int sig = 0; sig < 5; ++sig) vout[sig] = a.out[sig] && clip_aligned(a.out[sig] + row0);
#pragma unroll
  for (int k = 0; k < kMixGroups; ++k) {
    const int64_t j = c0 + 4 * (threadIdx.x + kMixThreads * k);
    if (j >= a.ld) break;
    float y[5][4];
#pragma unroll
    for (int sig = 0; sig < 5; ++sig)
#pragma unroll
      for (int e = 0; e < 4; ++e) y[sig][e] = 0.f;
    if (j < n) {
#pragma unroll
      for (int sig = 0; sig < 4; ++sig) {
        const bool need = a.in[sig] && (a.out[sig] || (a.out[MIX_MIXTURE] && (sig == MIX_NOISE || sig == speech_sig)));
        if (!need) continue;
        float x[4];
        clip_load(a.in[sig] + row0, vin[sig], j, n, x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j + e < n) y[sig][e] = ((sig == MIX_NOISE ? sc.noise(x[e]) : sc.speech(x[e])) * s2) * scale;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < n) y[MIX_MIXTURE][e] = y[MIX_NOISE][e] + (speech_sig == MIX_AUG ? y[MIX_AUG][e] : y[MIX_FRONT][e]);
    }
#pragma unroll
    for (int sig = 0; sig < 5; ++sig)
      if (a.out[sig]) clip_store(a.out[sig] + row0, vout[sig], j, a.ld, y[sig]);
  }
}

size_t mix_workspace_bytes(int B, int64_t lmax) {
  const size_t nb = (size_t)std::min(B, kMixMaxClips), nchunk = (size_t)((lmax + kClipChunk - 1) / kClipChunk);
  return nb * (kMixPeaks * sizeof(unsigned) + sizeof(MixLevel) + nchunk * 2 * sizeof(double));
}

void launch_mix_noise(int form, int B, int64_t ld, const int64_t* lengths, const float* const in[4], const double* noise_weight,
                      const double* scale, float* const out[5], char* ws, hipStream_t s) {
  const int64_t lmax = *std::max_element(lengths, lengths + B);
  const size_t nbmax = (size_t)std::min(B, kMixMaxClips);
  MixArgs a{};
  a.form = form;
  a.has_w = noise_weight != nullptr;
  a.ld = ld;
  a.nchunk = (int)((lmax + kClipChunk - 1) / kClipChunk);
  a.partial = reinterpret_cast<double*>(ws);  // (the widest alignment first)
  a.level = reinterpret_cast<MixLevel*>(ws + nbmax * a.nchunk * 2 * sizeof(double));
  a.peaks = reinterpret_cast<unsigned*>(ws + nbmax * (a.nchunk * 2 * sizeof(double) + sizeof(MixLevel)));
  for_clip_slices<kMixMaxClips>(B, [&](int b0, int nb) {  // the scratch is reused: the launches are ordered on the stream
    const int64_t nmax = narrow_clip_lengths(lengths, b0, nb, a.len);
    for (int i = 0; i < nb; ++i) {
      a.w[i] = noise_weight ? (float)noise_weight[b0 + i] : 1.f;
      a.scale[i] = (float)scale[b0 + i];
    }
    for (int sig = 0; sig < 4; ++sig) a.in[sig] = slice_rows(in[sig], b0, ld);
    for (int sig = 0; sig < 5; ++sig) a.out[sig] = slice_rows(out[sig], b0, ld);
    VFX_HIP(hipMemsetAsync(a.peaks, 0, (size_t)nb * kMixPeaks * sizeof(unsigned), s));
    const dim3 block(kMixThreads), grid((unsigned)((nmax + kClipChunk - 1) / kClipChunk), (unsigned)nb);
    hipLaunchKernelGGL(k_mix_peaks, grid, block, 0, s, a);
    VFX_HIP(hipGetLastError());
    if (form != 0) {
      hipLaunchKernelGGL(k_mix_sums, grid, block, 0, s, a);
      VFX_HIP(hipGetLastError());
      hipLaunchKernelGGL(k_mix_level, dim3((unsigned)nb), dim3(64), 0, s, a);
      VFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mix_mixpeak, grid, block, 0, s, a);
    VFX_HIP(hipGetLastError());
    const dim3 agrid((unsigned)((ld + kClipChunk - 1) / kClipChunk), (unsigned)nb);
    hipLaunchKernelGGL(k_mix_apply, agrid, block, 0, s, a);
    VFX_HIP(hipGetLastError());
  });
}

}  // namespace vfx
