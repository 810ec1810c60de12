// chain.hip -- the part of MagicalEffects' sox chain that is fully specified, for padded batches of float32 clips with a program per
// clip (gfx950): the four biquads (low_pass, high_pass, bass, treble), clip and reverse; mirrored by simulate.chain_effects, which a
// clip's result equals bit for bit.  Restated from published definitions, NOT pinned against sox.
//
// Arithmetic.  A sox run is a maximal stretch of biquads and reverses.  Entering it, the float32 clip is widened to float64 and
// limited to sox's sample range [-1, 1 - 2^-31]; a biquad is one transposed direct form II section from a zero state,
//
//   x_c = b0 x_n + z0;   z0 = (b1 x_n - a1 x_c) + z1;   z1 = b2 x_n - a2 x_c
//
// every product and sum rounded on its own (contraction is off in this file), and hands on limit(x_c) while its state keeps the
// unlimited x_c; reverse flips the clip; the run's result is rounded once to float32.  clip, between runs, clamps the float32 clip to
// [float32(min) float32(factor), float32(max) float32(factor)], float32 products, the minimum and maximum those of the clip as it
// stands.
//
// Passes.  chain_plan cuts a program into passes (ChainPass).  A pass reads the clip forward or backward, clamps what it reads to the
// bounds the pass before left, widens and limits, runs up to four biquads, rounds to float32 where the run ends, stores, and leaves
// the minimum and maximum of what it stored -- so a clip or a reverse in front of or behind a stretch of biquads costs no pass of its
// own.  What needs the whole clip first ends a pass: a clip step (its bounds), and a reverse between two biquads.  A pass with
// biquads is a cascade (k_chain_run); one without -- a program that starts with clip: the reduction; one that ends in clip or
// reverse: the last clamp or flip -- is element-wise (k_chain_map).  Round r of a slice of at most kChainMaxClips clips runs pass r of
// every clip that has one: ONE k_chain_run grid and ONE k_chain_map grid whatever the programs, never a launch per clip or per
// program.  Between passes a clip lives in one of two float64 scratch rows (a value rounded to float32 is stored exactly).
//
// k_chain_run is k_sosfilt_bank's forward pass without its padding, its initial state and its scratch: one lane per (clip, stage),
// a clip's stages in consecutive lanes of one 16-lane row, four clips per block; the cascade is skewed, stage s works on sample n - s
// and takes limit(x_c) of the stage below through row_shr:1; wave 0 runs the recurrence over one 64-sample LDS tile per clip while
// wave 1 stores the tile before and loads the next.  The clips of a block may have different stage counts.  k_chain_map is a grid
// over the batch in clip_batch.h's 16-byte sample groups.  A clip's result depends on the clip alone: not on the batch, the row
// stride, the alignment or its neighbours' programs.
//
// A sample that is not finite: the limit and the clamp are max-then-min, which send a NaN to their lower bound (the host form's
// np.clip keeps it); the statistics order bit patterns, where a NaN lies beyond the infinities.  What such a clip becomes is whatever
// that gives -- the list forms of simulate send it to the host function --; no other clip reads anything of it.
#include "clip_batch.h"
#include "vfx_internal.h"

#pragma clang fp contract(off)

namespace vfx {

constexpr int kChainTile = 64;              // samples per LDS tile of a clip (one wave-wide row)
constexpr int kChainRow = kChainTile + 1;   // doubles per LDS row: the pad spreads the clips' rows over the banks
constexpr int kChainBlockClips = 4;         // one per 16-lane row of the recurrence wave
constexpr int kChainMapThreads = 256;
constexpr int kChainGroup = 4;              // samples per thread and step of k_chain_map: one 16-byte group of float32
constexpr double kSoxLo = -1.0, kSoxHi = 1.0 - 1.0 / 2147483648.0;
static_assert(kChainMaxStages <= 16, "a clip's stages sit in one 16-lane row");

struct ChainArgs {
  const float* x;          // (clips, ldx)
  float* y;                // (clips, ldy)
  double* buf[2];          // (kChainMaxClips, lds) each
  const ChainPass* tab;
  unsigned* stats;         // [kChainMaxClips * kChainMaxPasses][2]: the order keys of the maximum and of the negated minimum
  int64_t ldx, ldy, lds;
  int n;                   // passes of this launch
  int idx[kChainMaxClips]; // their places in tab
};
static_assert(sizeof(ChainArgs) <= 1024, "the kernel-argument block");

// float32 values as unsigned keys of the same order (-0 below +0): the minimum and maximum of a clip by atomicMax
__device__ __forceinline__ unsigned chain_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float chain_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// (v_max_f64, v_min_f64: two instructions on the path from one stage to the next.  Two compares and two selects are eight, and were
// measured: 72 ns a step against 57)
__device__ __forceinline__ double chain_limit(double v) { return fmin(fmax(v, kSoxLo), kSoxHi); }

// a pass as its kernels use it (rows as offsets: the pointers stay the kernel's arguments, in global address space)
struct ChainIo {
  int64_t src_at, dst_at;  // the first sample of the source and of the destination row
  int len, S, stat_out;
  float lo, hi;
  uint8_t src, dst;        // ChainEnd
  bool rev, clamp, limit, round32, stats;
};

__device__ __forceinline__ ChainIo chain_io(const ChainArgs& a, const ChainPass& p) {
  ChainIo k;
  k.src = p.src, k.dst = p.dst;
  k.src_at = p.src == CHAIN_CALLER ? (int64_t)p.row * a.ldx : (int64_t)p.slot * a.lds;
  k.dst_at = p.dst == CHAIN_CALLER ? (int64_t)p.row * a.ldy : (int64_t)p.slot * a.lds;
  k.len = p.len;
  k.S = p.nbq;
  k.stat_out = p.stat_out;
  k.lo = k.hi = 0.0f;
  if (p.clamp) {  // float32 products, as x.min() * factor is
    k.lo = chain_unkey(~a.stats[2 * p.stat_in + 1]) * p.factor;
    k.hi = chain_unkey(a.stats[2 * p.stat_in]) * p.factor;
  }
  k.rev = p.rev, k.clamp = p.clamp, k.limit = p.limit, k.round32 = p.round32, k.stats = p.stats;
  return k;
}
__device__ __forceinline__ const double* chain_src(const ChainArgs& a, const ChainIo& k) {  // of a pass that reads the scratch
  return (k.src == CHAIN_BUF0 ? a.buf[0] : a.buf[1]) + k.src_at;
}
__device__ __forceinline__ double* chain_dst(const ChainArgs& a, const ChainIo& k) {  // of a pass that writes the scratch
  return (k.dst == CHAIN_BUF0 ? a.buf[0] : a.buf[1]) + k.dst_at;
}
__device__ __forceinline__ double chain_read(const ChainArgs& a, const ChainIo& k, int64_t i) {
  return k.src == CHAIN_CALLER ? (double)a.x[k.src_at + i] : chain_src(a, k)[i];
}

// what a pass makes of a sample it reads (every stored value that a clamp meets is a float32 value)
__device__ __forceinline__ double chain_enter(double v, const ChainIo& k) {
  if (k.clamp) v = (double)fminf(fmaxf((float)v, k.lo), k.hi);
  if (k.limit) v = chain_limit(v);
  return v;
}

struct ChainLane {
  double b0, b1, b2, a1, a2;  // the lane's stage
  double z0, z1, xc;          // its state, and what it hands on: its last output, limited
  int s;
  bool first, last;
};

// kChainTile steps of the skewed cascade over one LDS row per clip: sos_tile's arithmetic (sosfilt.hip) with the range limit on what
// a stage hands on.  WARM: the tile that starts a pass -- the lane of stage s starts at step s.
template <bool WARM>
__device__ __forceinline__ void chain_tile(double* row, ChainLane& L) {
  double xl = row[0];
#pragma unroll 4
  for (int i = 0; i < kChainTile; ++i) {
    const double below = row_shr1(L.xc);  // every lane takes part: a DPP move reads nothing from a lane that is masked off
    const double xin = L.first ? xl : below;
    xl = row[i + 1];  // (i = kChainTile - 1 reads the row's pad)
    const double xc = L.b0 * xin + L.z0;
    const double z0 = (L.b1 * xin - L.a1 * xc) + L.z1;
    const double z1 = L.b2 * xin - L.a2 * xc;
    if (!WARM || i >= L.s) {
      L.xc = chain_limit(xc);
      L.z0 = z0;
      L.z1 = z1;
    }
    if (L.last) row[i] = L.xc;
  }
}

__global__ __launch_bounds__(128) void k_chain_run(const ChainArgs a) {
  constexpr int C = kChainBlockClips;
  __shared__ __attribute__((aligned(16))) double smem[2 * C * kChainRow];
  __shared__ ChainIo io[C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * C;
  const int nc = min(C, a.n - c0);
  if (tid < nc) io[tid] = chain_io(a, a.tab[a.idx[c0 + tid]]);
  __syncthreads();
  int64_t steps = 0;  // of the skewed cascade over the clip that needs most
  for (int c = 0; c < nc; ++c) steps = max(steps, (int64_t)io[c].len + io[c].S - 1);
  const int ntiles = (int)((steps + kChainTile - 1) / kChainTile);

  // wave 1: one row of kChainTile samples per clip, lane i <-> sample i of the tile
  auto load_tile = [&](int t, int which) {
    double* const buf = smem + which * C * kChainRow;
    const int64_t n = (int64_t)t * kChainTile + lane;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (c >= nc) break;
      const ChainIo& k = io[c];
      double v = 0.0;
      if (n < k.len) {
        const int64_t i = k.rev ? k.len - 1 - n : n;
        v = chain_enter(chain_read(a, k, i), k);
      }
      buf[c * kChainRow + lane] = v;
    }
  };
  // slot i of tile t holds the cascade's output for sample t kChainTile + i - (S - 1) of the clip
  unsigned kmax[C], kmin[C];
#pragma unroll
  for (int c = 0; c < C; ++c) kmax[c] = kmin[c] = 0;
  auto flush_tile = [&](int t, int which) {
    const double* const buf = smem + which * C * kChainRow;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (c >= nc) break;
      const ChainIo& k = io[c];
      const int64_t p = (int64_t)t * kChainTile + lane - (k.S - 1);
      if (p < 0 || p >= k.len) continue;
      const double v = buf[c * kChainRow + lane];
      const float f = (float)v;
      if (k.dst == CHAIN_CALLER)
        a.y[k.dst_at + p] = f;
      else if (k.dst != CHAIN_NONE)
        chain_dst(a, k)[p] = k.round32 ? (double)f : v;
      kmax[c] = max(kmax[c], chain_key(f));
      kmin[c] = max(kmin[c], ~chain_key(f));
    }
  };

  // wave 0: lane -> (clip, stage) = (its 16-lane row, its place in the row); the lanes past S and the rows past nc idle along
  const int lc = lane >> 4;
  const bool active = lc < nc && (lane & 15) < io[lc < nc ? lc : 0].S;
  const int lcc = active ? lc : 0, s = active ? lane & 15 : 0;
  ChainLane L;
  L.s = s;
  L.first = s == 0;
  L.last = active && s == io[lcc].S - 1;
  L.b0 = L.b1 = L.b2 = L.a1 = L.a2 = 0.0;
  L.z0 = L.z1 = L.xc = 0.0;
  if (wave == 0) {
    if (active) {
      const double* const sec = a.tab[a.idx[c0 + lcc]].coef[s];
      L.b0 = sec[0], L.b1 = sec[1], L.b2 = sec[2], L.a1 = sec[3], L.a2 = sec[4];
    }
  } else {
    load_tile(0, 0);
  }
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    if (wave == 0) {
      double* const row = smem + ((t & 1) * C + lcc) * kChainRow;
      if (t == 0)
        chain_tile<true>(row, L);
      else
        chain_tile<false>(row, L);
    } else {
      if (t >= 1) flush_tile(t - 1, (t + 1) & 1);
      if (t + 1 < ntiles) load_tile(t + 1, (t + 1) & 1);
    }
    __syncthreads();
  }
  if (wave == 1) {
    flush_tile(ntiles - 1, (ntiles - 1) & 1);
#pragma unroll
    for (int c = 0; c < C; ++c) {  // a clip belongs to one block: its minimum and maximum are this wave's
      if (c >= nc || !io[c].stats) continue;
      unsigned hi = kmax[c], lo = kmin[c];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        hi = max(hi, (unsigned)__shfl_xor(hi, d));
        lo = max(lo, (unsigned)__shfl_xor(lo, d));
      }
      if (lane == 0) {
        atomicMax(a.stats + 2 * io[c].stat_out, hi);
        atomicMax(a.stats + 2 * io[c].stat_out + 1, lo);
      }
    }
  }
  for (int c = 0; c < nc; ++c) {  // zeros past the end of a clip that has arrived in y
    if (io[c].dst != CHAIN_CALLER) continue;
    float* const yr = a.y + io[c].dst_at;
    for (int64_t j = (int64_t)io[c].len + tid; j < a.ldy; j += 128) yr[j] = 0.0f;
  }
}

// samples [j, j + 4) of a pass's source as it reads them, j a multiple of 4; zeros at and past len
__device__ __forceinline__ void chain_load(const ChainArgs& a, const ChainIo& k, bool vec, int64_t j, double (&v)[kChainGroup]) {
  const int64_t n = k.len;
  if (k.rev) {
#pragma unroll
    for (int e = 0; e < kChainGroup; ++e) {
      const int64_t i = n - 1 - (j + e);
      v[e] = i < 0 ? 0.0 : chain_read(a, k, i);
    }
  } else if (k.src == CHAIN_CALLER) {
    float f[kChainGroup];
    clip_load(a.x + k.src_at, vec, j, n, f);
#pragma unroll
    for (int e = 0; e < kChainGroup; ++e) v[e] = (double)f[e];
  } else {
    double d[2];
#pragma unroll
    for (int g = 0; g < kChainGroup; g += 2) {
      clip_load(chain_src(a, k), vec, j + g, n, d);
      v[g] = d[0], v[g + 1] = d[1];
    }
  }
}

__global__ __launch_bounds__(kChainMapThreads) void k_chain_map(const ChainArgs a) {
  constexpr int G = kChainGroup, K = kClipChunk / (G * kChainMapThreads);
  static_assert(kClipChunk == G * kChainMapThreads * K, "a chunk is whole groups of every thread");
  const ChainIo k = chain_io(a, a.tab[a.idx[blockIdx.y]]);
  const int64_t n = k.len, c0 = (int64_t)blockIdx.x * kClipChunk;
  const bool to_y = k.dst == CHAIN_CALLER;
  const int64_t extent = to_y ? a.ldy : n;  // a row of y is zeroed up to ldy
  if (c0 >= extent) return;
  const bool vin = k.src == CHAIN_CALLER ? clip_aligned(a.x + k.src_at) : clip_aligned(chain_src(a, k));
  const bool vout = to_y ? clip_aligned(a.y + k.dst_at) : (k.dst != CHAIN_NONE && clip_aligned(chain_dst(a, k)));
  unsigned kmax = 0, kmin = 0;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const int64_t j = c0 + G * (threadIdx.x + kChainMapThreads * q);
    if (j >= extent) break;
    float f[G];
    double d[G];
#pragma unroll
    for (int e = 0; e < G; ++e) f[e] = 0.0f, d[e] = 0.0;
    if (j < n) {
      double v[G];
      chain_load(a, k, vin, j, v);
#pragma unroll
      for (int e = 0; e < G; ++e) {
        if (j + e >= n) continue;
        const double w = chain_enter(v[e], k);
        f[e] = (float)w;
        d[e] = k.round32 ? (double)f[e] : w;
        kmax = max(kmax, chain_key(f[e]));
        kmin = max(kmin, ~chain_key(f[e]));
      }
    }
    if (to_y)
      clip_store(a.y + k.dst_at, vout, j, a.ldy, f);
    else if (k.dst != CHAIN_NONE)
      clip_store(chain_dst(a, k), vout, j, a.lds, d);
  }
  if (k.stats) {  // (the same for every thread of the workgroup)
    __shared__ unsigned slots[2][kChainMapThreads / 64];
    clip_commit_peak<kChainMapThreads>(kmax, a.stats + 2 * k.stat_out, slots[0]);
    clip_commit_peak<kChainMapThreads>(kmin, a.stats + 2 * k.stat_out + 1, slots[1]);
  }
}

void chain_plan(int B, const int64_t* lengths, const int* ops, const double* coef, int K, std::vector<ChainPass>& passes,
                std::vector<int>& first) {
  passes.clear();
  first.assign(1, 0);
  for (int b = 0; b < B; ++b) {
    const int* const o = ops + (size_t)b * K;
    const double* const cf = coef + (size_t)b * K * 5;
    int nops = 0, in_run = 0;
    for (; nops < K && o[nops] != VFX_CHAIN_END; ++nops) {
      const int op = o[nops];
      VFX_CHECK(op == VFX_CHAIN_BIQUAD || op == VFX_CHAIN_CLIP || op == VFX_CHAIN_REVERSE, "vfx_effect_chain: clip %d: step %d is op %d", b,
                nops, op);
      in_run = op == VFX_CHAIN_CLIP ? 0 : in_run + (op == VFX_CHAIN_BIQUAD);
      VFX_CHECK(in_run <= kChainMaxStages, "vfx_effect_chain: clip %d: more than %d biquads in one run (step %d)", b, kChainMaxStages, nops);
    }
    const int slot = b % kChainMaxClips;
    uint8_t src = CHAIN_CALLER, next = CHAIN_BUF0;
    auto emit = [&](ChainPass c, bool round32, bool stats, uint8_t dst) {
      c.row = b, c.slot = slot, c.len = (int)lengths[b];
      c.stat_out = slot * kChainMaxPasses + ((int)passes.size() - first[b]);
      c.stat_in = c.stat_out - 1;
      c.round32 = round32, c.stats = stats, c.src = src, c.dst = dst;
      if (dst == CHAIN_BUF0 || dst == CHAIN_BUF1) src = dst, next = dst == CHAIN_BUF0 ? CHAIN_BUF1 : CHAIN_BUF0;
      passes.push_back(c);
    };
    ChainPass cur{};
    bool flip_behind = false;  // a reverse behind cur's biquads: the next pass reads backward
    auto pending = [&] { return cur.nbq || cur.rev || cur.clamp || cur.limit; };
    for (int k = 0; k < nops; ++k) {
      if (o[k] == VFX_CHAIN_BIQUAD) {
        if (flip_behind) {  // the run goes on behind the flip: the clip stays float64
          emit(cur, false, false, next);
          cur = ChainPass{};
          cur.rev = 1;
          flip_behind = false;
        }
        cur.limit = 1;
        std::copy(cf + k * 5, cf + k * 5 + 5, cur.coef[cur.nbq++]);
      } else if (o[k] == VFX_CHAIN_REVERSE) {
        if (cur.nbq)
          flip_behind = !flip_behind;
        else
          cur.rev ^= 1, cur.limit = 1;  // (a run of reverses alone still limits and rounds)
      } else {  // a clip step needs the minimum and maximum of the clip as it stands; it commutes with a flip
        if (pending())
          emit(cur, true, true, next);
        else
          emit(ChainPass{}, true, true, CHAIN_NONE);  // the program starts with clip: the reduction over x
        cur = ChainPass{};
        cur.clamp = 1;
        cur.factor = (float)cf[k * 5];
        cur.rev = flip_behind;
        flip_behind = false;
      }
    }
    if (flip_behind) {
      emit(cur, true, false, next);
      cur = ChainPass{};
      cur.rev = 1;
    }
    emit(cur, true, false, CHAIN_CALLER);  // (an empty program: the copy)
    first.push_back((int)passes.size());
  }
}

void launch_effect_chain(const float* x, int64_t ldx, int B, const std::vector<ChainPass>& passes, const std::vector<int>& first,
                         const ChainPass* tab, double* buf0, double* buf1, int64_t lds, unsigned* stats, float* y, int64_t ldy,
                         hipStream_t s) {
  ChainArgs run{}, map{};
  run.x = x, run.y = y, run.buf[0] = buf0, run.buf[1] = buf1, run.tab = tab, run.stats = stats;
  run.ldx = ldx, run.ldy = ldy, run.lds = lds;
  map = run;
  for_clip_slices<kChainMaxClips>(B, [&](int b0, int nb) {  // x and y stay whole: ChainPass::row is the caller's row
    int rounds = 0;
    bool any_stats = false;
    for (int b = b0; b < b0 + nb; ++b) {
      rounds = std::max(rounds, first[b + 1] - first[b]);
      for (int i = first[b]; i < first[b + 1]; ++i) any_stats |= passes[i].stats != 0;
    }
    if (any_stats) VFX_HIP(hipMemsetAsync(stats, 0, (size_t)kChainMaxClips * kChainMaxPasses * 2 * sizeof(unsigned), s));
    for (int r = 0; r < rounds; ++r) {
      run.n = map.n = 0;
      int64_t extent = 0;  // of the element-wise grid: a clip, or a row of y
      for (int b = b0; b < b0 + nb; ++b) {
        const int i = first[b] + r;
        if (i >= first[b + 1]) continue;
        if (passes[i].nbq) {
          run.idx[run.n++] = i;
        } else {
          map.idx[map.n++] = i;
          extent = std::max(extent, passes[i].dst == CHAIN_CALLER ? ldy : (int64_t)passes[i].len);
        }
      }
      if (run.n) {
        hipLaunchKernelGGL(k_chain_run, dim3((unsigned)((run.n + kChainBlockClips - 1) / kChainBlockClips)), dim3(128), 0, s, run);
        VFX_HIP(hipGetLastError());
      }
      if (map.n) {
        hipLaunchKernelGGL(k_chain_map, dim3((unsigned)((extent + kClipChunk - 1) / kClipChunk), (unsigned)map.n), dim3(kChainMapThreads), 0,
                           s, map);
        VFX_HIP(hipGetLastError());
      }
    }
  });
}

}  // namespace vfx
