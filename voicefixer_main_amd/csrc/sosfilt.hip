// sosfilt.hip -- batched zero-phase IIR filter (gfx950), bit-identical to scipy.signal.sosfiltfilt(sos, x) on float32 / float64 input.
//
// sosfiltfilt extends a clip oddly by padlen samples at each end IN THE CLIP'S DTYPE (ext = [2 x[0] - x[padlen:0:-1], x,
// 2 x[-1] - x[-2:-padlen-2:-1]]), widens to float64, runs the cascade of S second-order sections forward over ext from the state
// zi * ext[0], runs it again over the forward result read from its last sample to its first from the state zi * (that last sample),
// reverses, and drops the padlen samples at each end.  Per sample and section (transposed direct form II, a0 = 1), in float64 with
// every product and sum rounded on its own:
//
//   x_c = b0 x_n + z0;   z0 = (b1 x_n - a1 x_c) + z1;   z1 = b2 x_n - a2 x_c;   the section's output is x_c
//
// Contraction is off in this file, so the kernel does exactly those roundings (tests/test_gpu_sosfiltfilt.py compares with
// torch.equal).
//
// Lane mapping: one lane per (clip, section).  A clip's S sections sit in consecutive lanes of one 16-lane row, 16 / S clips per row
// (at most 8), four rows per wave.  The cascade is skewed: at step n the lane of section s works on sample n - s, and takes its input
// from the lane below it (a row_shr:1 DPP move of the previous step's x_c); section 0 reads its sample from LDS, the last section
// writes its output over it.  A block is two waves: wave 0 runs the recurrence over one 64-sample tile of every clip while wave 1
// writes the previous tile's outputs to global memory and fetches the next tile's inputs -- one coalesced row of 64 samples per
// clip -- into the other LDS buffer; the waves meet at one barrier per tile.  The loop-carried chain per step is the four dependent
// float64 operations of the z0 update, whatever the batch size: the pass is latency-bound, parallel over clips x sections only.
#include "clip_batch.h"
#include "vfx_internal.h"

#pragma clang fp contract(off)

namespace vfx {

constexpr int kSosRow = kSosTile + 1;  // doubles per LDS row: the pad spreads the clips' rows over the banks

struct SosArgs {
  const void* x;  // (clips, ldx) float32 or float64
  double* f;      // (clips, ldf): the forward pass over the extended clips
  double* y;      // (clips, ldy)
  int64_t ldx, ldf, ldy;
  int x_f64, bwd, B, S, cpr, C, padlen;
  double sos[kSosMaxSections][5];  // b0 b1 b2 a1 a2
  double zi[kSosMaxSections][2];
  int len[kSosMaxClips];
};

// sample n of the odd extension of x[0 .. len), 0 <= n < len + 2 padlen, len > padlen: computed in T, then widened
template <typename T>
__device__ inline double ext_at(const T* x, int64_t len, int padlen, int64_t n) {
  if (n < padlen) return (double)(T(2) * x[0] - x[padlen - n]);
  n -= padlen;
  if (n < len) return (double)x[n];
  n -= len;
  return (double)(T(2) * x[len - 1] - x[len - 2 - n]);
}

struct SosLane {
  double b0, b1, b2, a1, a2;  // the lane's section
  double z0, z1, xc;          // its state and its last output
  int s;
  bool first, last;
};

// kSosTile steps of the skewed cascade over one LDS row per clip.  WARM: the tile that starts a pass -- the lane of section s
// starts at step s.
template <bool WARM>
__device__ __forceinline__ void sos_tile(double* row, SosLane& L) {
  double xl = row[0];
#pragma unroll 4
  for (int i = 0; i < kSosTile; ++i) {
    const double below = row_shr1(L.xc);  // every lane takes part: a DPP move reads nothing from a lane that is masked off
    const double xin = L.first ? xl : below;
    xl = row[i + 1];  // (i = kSosTile - 1 reads the row's pad)
    const double xc = L.b0 * xin + L.z0;
    const double z0 = (L.b1 * xin - L.a1 * xc) + L.z1;
    const double z1 = L.b2 * xin - L.a2 * xc;
    if (!WARM || i >= L.s) {
      L.xc = xc;
      L.z0 = z0;
      L.z1 = z1;
    }
    if (L.last) row[i] = L.xc;
  }
}

__global__ __launch_bounds__(128) void k_sosfilt(const SosArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sos_smem[];  // [2][C][kSosRow]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, C = a.C, padlen = a.padlen;
  const bool bwd = a.bwd != 0;
  const int c0 = blockIdx.x * C;
  const int nc = min(C, a.B - c0);
  int maxlen = 0;
  for (int c = 0; c < nc; ++c) maxlen = max(maxlen, a.len[c0 + c]);
  // steps of the skewed cascade over the longest clip; the backward pass stops where its last kept output is done
  const int64_t steps = (int64_t)maxlen + (bwd ? padlen : 2 * padlen) + S - 1;
  const int ntiles = (int)((steps + kSosTile - 1) / kSosTile);

  // wave 1: one row of kSosTile samples per clip, lane i <-> sample i of the tile
  auto load_tile = [&](int t, int which) {
    double* const buf = sos_smem + which * C * kSosRow;
    const int64_t n = (int64_t)t * kSosTile + lane;
#pragma unroll 4
    for (int c = 0; c < nc; ++c) {
      const int64_t len = a.len[c0 + c], lext = len + 2 * padlen;
      double v = 0.0;
      if (n < lext) {
        if (bwd)
          v = a.f[(int64_t)(c0 + c) * a.ldf + (lext - 1 - n)];
        else if (a.x_f64)
          v = ext_at(static_cast<const double*>(a.x) + (int64_t)(c0 + c) * a.ldx, len, padlen, n);
        else
          v = ext_at(static_cast<const float*>(a.x) + (int64_t)(c0 + c) * a.ldx, len, padlen, n);
      }
      buf[c * kSosRow + lane] = v;
    }
  };
  // slot i of tile t holds the cascade's output for position t kSosTile + i - (S - 1) of the pass
  auto flush_tile = [&](int t, int which) {
    const double* const buf = sos_smem + which * C * kSosRow;
    const int64_t p = (int64_t)t * kSosTile + lane - (S - 1);
#pragma unroll 4
    for (int c = 0; c < nc; ++c) {
      const int64_t len = a.len[c0 + c], lext = len + 2 * padlen;
      const double v = buf[c * kSosRow + lane];
      if (bwd) {
        const int64_t q = lext - 1 - p - padlen;  // index in the clip
        if (p >= 0 && q >= 0 && q < len) a.y[(int64_t)(c0 + c) * a.ldy + q] = v;
      } else if (p >= 0 && p < lext) {
        a.f[(int64_t)(c0 + c) * a.ldf + p] = v;
      }
    }
  };

  // wave 0: lane -> (clip, section)
  const int r = lane & 15;
  const int cin = r / S, s = r - cin * S;
  const int lc = (lane >> 4) * a.cpr + cin;
  const bool active = cin < a.cpr && lc < nc;
  const int lcc = active ? lc : 0;
  SosLane L;
  L.s = s;
  L.first = s == 0;
  L.last = active && s == S - 1;
  L.b0 = a.sos[s][0], L.b1 = a.sos[s][1], L.b2 = a.sos[s][2], L.a1 = a.sos[s][3], L.a2 = a.sos[s][4];
  L.z0 = L.z1 = L.xc = 0.0;
  if (wave == 0) {
    const int64_t len = a.len[c0 + lcc], lext = len + 2 * padlen;
    double x0;
    if (bwd)
      x0 = a.f[(int64_t)(c0 + lcc) * a.ldf + lext - 1];
    else if (a.x_f64)
      x0 = ext_at(static_cast<const double*>(a.x) + (int64_t)(c0 + lcc) * a.ldx, len, padlen, 0);
    else
      x0 = ext_at(static_cast<const float*>(a.x) + (int64_t)(c0 + lcc) * a.ldx, len, padlen, 0);
    L.z0 = a.zi[s][0] * x0;
    L.z1 = a.zi[s][1] * x0;
  } else {
    load_tile(0, 0);
  }
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    if (wave == 0) {
      double* const row = sos_smem + ((t & 1) * C + lcc) * kSosRow;
      if (t == 0)
        sos_tile<true>(row, L);
      else
        sos_tile<false>(row, L);
    } else {
      if (t >= 1) flush_tile(t - 1, (t + 1) & 1);
      if (t + 1 < ntiles) load_tile(t + 1, (t + 1) & 1);
    }
    __syncthreads();
  }
  if (wave == 1) flush_tile(ntiles - 1, (ntiles - 1) & 1);
  if (bwd) {  // zeros past each clip's end
    for (int c = 0; c < nc; ++c) {
      double* const yr = a.y + (int64_t)(c0 + c) * a.ldy;
      for (int64_t j = (int64_t)a.len[c0 + c] + tid; j < a.ldy; j += 128) yr[j] = 0.0;
    }
  }
}

int sosfilt_clips_per_wave(int S) { return 4 * std::min(16 / S, 8); }

void launch_sosfiltfilt(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const double* sos, int S, const double* zi,
                        int padlen, double* f, int64_t ldf, double* y, int64_t ldy, hipStream_t s) {
  VFX_CHECK(S >= 1 && S <= kSosMaxSections, "sosfiltfilt: %d sections (1 .. %d)", S, kSosMaxSections);
  SosArgs a{};
  a.ldx = ldx;
  a.ldf = ldf;
  a.ldy = ldy;
  a.x_f64 = x_f64;
  a.S = S;
  a.cpr = std::min(16 / S, 8);
  a.C = 4 * a.cpr;
  a.padlen = padlen;
  for (int i = 0; i < S; ++i) {
    a.sos[i][0] = sos[i * 6 + 0];
    a.sos[i][1] = sos[i * 6 + 1];
    a.sos[i][2] = sos[i * 6 + 2];
    a.sos[i][3] = sos[i * 6 + 4];
    a.sos[i][4] = sos[i * 6 + 5];
    a.zi[i][0] = zi[i * 2 + 0];
    a.zi[i][1] = zi[i * 2 + 1];
  }
  const size_t lds = (size_t)2 * a.C * kSosRow * sizeof(double);  // at most 33 280 bytes
  const size_t elt = x_f64 ? sizeof(double) : sizeof(float);
  a.f = f;  // the scratch is reused: the launches are ordered on the stream
  for_clip_slices<kSosMaxClips>(B, [&](int b0, int nb) {
    a.B = nb;
    a.x = slice_rows(x, b0, ldx, elt);
    a.y = slice_rows(y, b0, ldy);
    narrow_clip_lengths(lengths, b0, nb, a.len);
    const dim3 grid((unsigned)((a.B + a.C - 1) / a.C));
    for (int bwd = 0; bwd < 2; ++bwd) {
      a.bwd = bwd;
      hipLaunchKernelGGL(k_sosfilt, grid, dim3(128), lds, s, a);
      VFX_HIP(hipGetLastError());
    }
  });
}

// ---------------------------------------------------------------------------------------------
// The bank form: every clip has its own design.  k_sosfilt's lane mapping needs one section count per block, so the launcher orders
// the clips of a launch by section count and a block owns up to kSosBankBlockClips clips of ONE count -- its descriptor says which.
// Blocks of different counts run side by side in one grid: the pass is latency-bound, a launch per count would multiply its time.
// A clip has a 16-lane row of the recurrence wave to itself, whatever S: wave 1 moves a block's clips one after the other, and
// with more than about six of them it, not the recurrence, sets the block's time (DESIGN.md has the measurement), while a launch
// of kSosMaxClips clips is 48 blocks at most either way.  x and y keep the caller's row order (SosClip::row); the forward scratch
// is indexed by the clip's place in the launch.  Coefficients and zi come from the bank in device memory, read once per lane.  The
// arithmetic is sos_tile's and ext_at's, as in k_sosfilt.
// ---------------------------------------------------------------------------------------------
constexpr int kSosBankBlockClips = 4;  // one per 16-lane row of the recurrence wave
static_assert(kSosMaxBlocks >= kSosMaxClips / kSosBankBlockClips + kSosMaxSections, "full blocks + one partial block per section count");
struct SosBlock {
  uint8_t S, first, count;  // section count, the block's clips [first, first + count) of the launch
};
struct SosClip {
  int row, len;             // row of x and y; samples
  uint16_t padlen, design;  // of its design; index into the bank
};
struct SosBankArgs {
  const void* x;
  double* f;
  double* y;
  const double* bank;  // (F, Smax, kSosBankRow)
  int64_t ldx, ldf, ldy;
  int x_f64, bwd, Smax;
  SosBlock blk[kSosMaxBlocks];
  SosClip clip[kSosMaxClips];
};
static_assert(sizeof(SosBankArgs) <= 2048, "the kernel-argument block");
static_assert(kSosMaxClips <= 256 && kSosMaxDesigns <= 65536, "SosBlock::first, SosClip::design");

__global__ __launch_bounds__(128) void k_sosfilt_bank(const SosBankArgs a) {
  constexpr int C = kSosBankBlockClips;
  __shared__ __attribute__((aligned(16))) double sos_smem[2 * C * kSosRow];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SosBlock d = a.blk[blockIdx.x];
  const int S = d.S, c0 = d.first, nc = d.count;
  const bool bwd = a.bwd != 0;
  int64_t steps = 0;  // of the skewed cascade over the clip that needs most; the backward pass stops where its last kept output is done
  for (int c = 0; c < nc; ++c) steps = max(steps, (int64_t)a.clip[c0 + c].len + (bwd ? 1 : 2) * (int)a.clip[c0 + c].padlen);
  steps += S - 1;
  const int ntiles = (int)((steps + kSosTile - 1) / kSosTile);

  // wave 1: one row of kSosTile samples per clip, lane i <-> sample i of the tile
  auto load_tile = [&](int t, int which) {
    double* const buf = sos_smem + which * C * kSosRow;
    const int64_t n = (int64_t)t * kSosTile + lane;
#pragma unroll 4
    for (int c = 0; c < nc; ++c) {
      const SosClip k = a.clip[c0 + c];
      const int64_t len = k.len, lext = len + 2 * (int)k.padlen;
      double v = 0.0;
      if (n < lext) {
        if (bwd)
          v = a.f[(int64_t)(c0 + c) * a.ldf + (lext - 1 - n)];
        else if (a.x_f64)
          v = ext_at(static_cast<const double*>(a.x) + (int64_t)k.row * a.ldx, len, (int)k.padlen, n);
        else
          v = ext_at(static_cast<const float*>(a.x) + (int64_t)k.row * a.ldx, len, (int)k.padlen, n);
      }
      buf[c * kSosRow + lane] = v;
    }
  };
  // slot i of tile t holds the cascade's output for position t kSosTile + i - (S - 1) of the pass
  auto flush_tile = [&](int t, int which) {
    const double* const buf = sos_smem + which * C * kSosRow;
    const int64_t p = (int64_t)t * kSosTile + lane - (S - 1);
#pragma unroll 4
    for (int c = 0; c < nc; ++c) {
      const SosClip k = a.clip[c0 + c];
      const int64_t len = k.len, lext = len + 2 * (int)k.padlen;
      const double v = buf[c * kSosRow + lane];
      if (bwd) {
        const int64_t q = lext - 1 - p - (int)k.padlen;  // index in the clip
        if (p >= 0 && q >= 0 && q < len) a.y[(int64_t)k.row * a.ldy + q] = v;
      } else if (p >= 0 && p < lext) {
        a.f[(int64_t)(c0 + c) * a.ldf + p] = v;
      }
    }
  };

  // wave 0: lane -> (clip, section) = (its 16-lane row, its place in the row); the lanes past S and the rows past nc idle along
  const int lc = lane >> 4;
  const bool active = (lane & 15) < S && lc < nc;
  const int lcc = active ? lc : 0, s = active ? lane & 15 : 0;
  SosLane L;
  L.s = s;
  L.first = s == 0;
  L.last = active && s == S - 1;
  L.b0 = L.b1 = L.b2 = L.a1 = L.a2 = 0.0;
  L.z0 = L.z1 = L.xc = 0.0;
  if (wave == 0) {
    const SosClip k = a.clip[c0 + lcc];
    const double* const sec = a.bank + ((int64_t)k.design * a.Smax + s) * kSosBankRow;
    L.b0 = sec[0], L.b1 = sec[1], L.b2 = sec[2], L.a1 = sec[3], L.a2 = sec[4];
    const int64_t len = k.len, lext = len + 2 * (int)k.padlen;
    double x0;
    if (bwd)
      x0 = a.f[(int64_t)(c0 + lcc) * a.ldf + lext - 1];
    else if (a.x_f64)
      x0 = ext_at(static_cast<const double*>(a.x) + (int64_t)k.row * a.ldx, len, (int)k.padlen, 0);
    else
      x0 = ext_at(static_cast<const float*>(a.x) + (int64_t)k.row * a.ldx, len, (int)k.padlen, 0);
    L.z0 = sec[5] * x0;
    L.z1 = sec[6] * x0;
  } else {
    load_tile(0, 0);
  }
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    if (wave == 0) {
      double* const row = sos_smem + ((t & 1) * C + lcc) * kSosRow;
      if (t == 0)
        sos_tile<true>(row, L);
      else
        sos_tile<false>(row, L);
    } else {
      if (t >= 1) flush_tile(t - 1, (t + 1) & 1);
      if (t + 1 < ntiles) load_tile(t + 1, (t + 1) & 1);
    }
    __syncthreads();
  }
  if (wave == 1) flush_tile(ntiles - 1, (ntiles - 1) & 1);
  if (bwd) {  // zeros past each clip's end
    for (int c = 0; c < nc; ++c) {
      double* const yr = a.y + (int64_t)a.clip[c0 + c].row * a.ldy;
      for (int64_t j = (int64_t)a.clip[c0 + c].len + tid; j < a.ldy; j += 128) yr[j] = 0.0;
    }
  }
}

void sosfilt_pack_bank(const double* sos, const double* zi, int F, int Smax, double* bank) {
  for (int i = 0; i < F * Smax; ++i) {
    const double row[kSosBankRow] = {sos[i * 6 + 0], sos[i * 6 + 1], sos[i * 6 + 2], sos[i * 6 + 4], sos[i * 6 + 5], zi[i * 2 + 0], zi[i * 2 + 1]};
    std::copy(row, row + kSosBankRow, bank + (size_t)i * kSosBankRow);
  }
}

void launch_sosfiltfilt_bank(const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* filter_index,
                             const double* bank, int Smax, const int* sections, const int* padlens, double* f, int64_t ldf, double* y,
                             int64_t ldy, hipStream_t s) {
  SosBankArgs a{};
  a.x = x;
  a.f = f;  // the scratch is reused: the launches are ordered on the stream
  a.y = y;
  a.bank = bank;
  a.ldx = ldx;
  a.ldf = ldf;
  a.ldy = ldy;
  a.x_f64 = x_f64;
  a.Smax = Smax;
  for_clip_slices<kSosMaxClips>(B, [&](int b0, int n) {  // x and y stay whole: SosClip::row is the caller's row
    int order[kSosMaxClips];
    for (int i = 0; i < n; ++i) order[i] = b0 + i;
    std::stable_sort(order, order + n, [&](int p, int q) { return sections[filter_index[p]] < sections[filter_index[q]]; });
    int nblk = 0;
    for (int j = 0; j < n; ++j) {
      const int b = order[j], fi = filter_index[b], S = sections[fi];
      VFX_CHECK(S >= 1 && S <= kSosMaxSections && S <= Smax, "sosfiltfilt bank: design %d has %d sections (1 .. %d)", fi, S,
                std::min(Smax, kSosMaxSections));
      a.clip[j] = SosClip{b, (int)lengths[b], (uint16_t)padlens[fi], (uint16_t)fi};
      if (nblk == 0 || a.blk[nblk - 1].S != S || a.blk[nblk - 1].count == kSosBankBlockClips) {
        VFX_CHECK(nblk < kSosMaxBlocks, "sosfiltfilt bank: more than %d blocks", kSosMaxBlocks);
        a.blk[nblk++] = SosBlock{(uint8_t)S, (uint8_t)j, 0};
      }
      ++a.blk[nblk - 1].count;
    }
    for (int bwd = 0; bwd < 2; ++bwd) {
      a.bwd = bwd;
      hipLaunchKernelGGL(k_sosfilt_bank, dim3((unsigned)nblk), dim3(128), 0, s, a);
      VFX_HIP(hipGetLastError());
    }
  });
}

}  // namespace vfx
