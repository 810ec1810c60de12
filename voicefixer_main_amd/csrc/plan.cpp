// plan.cpp -- device allocations, launch geometry, plan building, binding and running.
#include <cmath>
#include <cstring>
#include <cstdlib>

#include "vfx_internal.h"

namespace vfx {

// ---------------------------------------------------------------------------------------------
// device blob / arena planner
// ---------------------------------------------------------------------------------------------
void* DeviceBlob::alloc(size_t bytes) {
  void* p = nullptr;
  VFX_HIP(hipMalloc(&p, bytes ? bytes : 16));
  allocs.push_back(p);
  return p;
}
float* DeviceBlob::upload(const float* p, size_t n) {
  float* d = static_cast<float*>(alloc(n * sizeof(float)));
  if (n) VFX_HIP(hipMemcpy(d, p, n * sizeof(float), hipMemcpyHostToDevice));
  return d;
}
int* DeviceBlob::upload_i(const std::vector<int>& v) {
  int* d = static_cast<int*>(alloc(v.size() * sizeof(int)));
  if (!v.empty()) VFX_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
  return d;
}
void DeviceBlob::release() {
  for (void* p : allocs) (void)hipFree(p);
  allocs.clear();
}

size_t ArenaPlanner::alloc(size_t bytes) {
  bytes = (bytes + 255) & ~size_t(255);
  if (bytes == 0) bytes = 256;
  for (size_t i = 0; i < blocks.size(); ++i) {
    Block& b = blocks[i];
    if (b.free && b.size >= bytes) {
      if (b.size > bytes) {
        Block rest{b.off + bytes, b.size - bytes, true};
        b.size = bytes;
        b.free = false;
        const size_t off = b.off;
        blocks.insert(blocks.begin() + i + 1, rest);
        return off;
      }
      b.free = false;
      return b.off;
    }
  }
  // extend: merge with a trailing free block if there is one
  if (!blocks.empty() && blocks.back().free) {
    Block& b = blocks.back();
    b.size = bytes;
    b.free = false;
    high = b.off + bytes;
    return b.off;
  }
  blocks.push_back(Block{high, bytes, false});
  const size_t off = high;
  high += bytes;
  return off;
}

void ArenaPlanner::free(size_t off) {
  for (size_t i = 0; i < blocks.size(); ++i) {
    if (blocks[i].off == off && !blocks[i].free) {
      blocks[i].free = true;
      if (i + 1 < blocks.size() && blocks[i + 1].free) {
        blocks[i].size += blocks[i + 1].size;
        blocks.erase(blocks.begin() + i + 1);
      }
      if (i > 0 && blocks[i - 1].free) {
        blocks[i - 1].size += blocks[i].size;
        blocks.erase(blocks.begin() + i);
      }
      return;
    }
  }
  set_error("ArenaPlanner::free: unknown offset %zu", off);
  throw Error();
}

// Tile and patch geometry of a launch.  The tile is TH x TW <= 128 pixels of one image; if the
// bounding box of all taps around it fits kPatchMaxRows pixels, every (segment, chunk) is ONE stage
// reading all its taps from one patch; otherwise (Conv1d with dilation > 48) every (chunk, tap)
// is its own stage with a tile-sized patch.
static void plan_conv(TapConvParams& p) {
  int dh_lo = 1 << 30, dh_hi = -(1 << 30), dw_lo = 1 << 30, dw_hi = -(1 << 30);
  for (int s = 0; s < p.nseg; ++s)
    for (int t = 0; t < p.seg[s].ntaps; ++t) {
      dh_lo = std::min(dh_lo, p.seg[s].dh[t]);
      dh_hi = std::max(dh_hi, p.seg[s].dh[t]);
      dw_lo = std::min(dw_lo, p.seg[s].dw[t]);
      dw_hi = std::max(dw_hi, p.seg[s].dw[t]);
    }
  bool bodies_ok = true;  // conv.hip instantiates stage bodies for these tap counts only
  for (int s = 0; s < p.nseg; ++s) {
    const int nt = p.seg[s].ntaps;
    bodies_ok = bodies_ok && (nt == 1 || nt == 2 || nt == 3 || nt == 4 || nt == 7 || nt == 9);
  }
  // Tile shape: TW = 2^k columns x TH = min(128 / TW, Hg) rows.  Among the shapes whose all-taps window
  // fits kPatchMaxRows pixels take the one that wastes the fewest tile pixels on the image borders
  // (ties: the smaller window); if none fits, fall back to one stage per (chunk, tap) with a tile-sized patch.
  int best_shift = -1;
  double best_util = -1.0;
  int64_t best_P = 0;
  const int sft0 = p.Hg == 1 ? 7 : 0;
  // Rows of a TW-wide tile: 128 / TW, the image's height, and -- round 5 -- what keeps the all-taps window inside the patch
  // buffer.  A TALL NARROW image (level 6 of a 60-s segment: 188 x 3 pixels; the bottleneck: 94 x 1) had no shape at all whose
  // window fits at 128 / TW rows and fell back to one stage per (chunk, tap): nine times the stages, no split-K, 0.13 - 0.36 ms
  // per launch where a 16 x 10 s batch takes 0.05 (profiles/r05_1x60_vs_16x10_per_launch.txt).  Shapes that fitted before keep
  // their rows.
  // Round 6: an image NARROWER than the tile (level 6 of the mel ResUNet: 3 columns on 4-wide tiles) stages only the columns it has --
  // window width min(TW, Wg) + taps instead of TW + taps: 34 x 5 = 170 patch pixels hold all 32 rows of a 10-s clip's level 6 in ONE tile
  // (34 x 6 = 204 did not fit: two tiles of 30 + 2 rows, i.e. 1 536 blocks = two rounds of the chip's 768 slots per launch, 44-55 us
  // where one round takes 24-26).  The tile's dead columns read rows of the neighbouring patch pixels (the `dead` slack keeps them
  // inside the buffer) into accumulator columns nobody stores.
  auto win_w = [&](int TW) { return (int64_t)std::min(TW, p.Wg) + (int64_t)(dw_hi - dw_lo); };
  auto rows_of = [&](int sft) {
    const int TW = 1 << sft;
    const int64_t PW = win_w(TW), dead = TW - std::min(TW, p.Wg);
    const int64_t fit = (kPatchMaxRows - dead) / PW - (int64_t)(dh_hi - dh_lo);
    return (int)std::max<int64_t>(0, std::min<int64_t>(std::min(128 / TW, p.Hg), fit));
  };
  for (int sft = sft0; sft <= 7; ++sft) {
    const int TW = 1 << sft, TH = rows_of(sft);
    if (TW > 2 * p.Wg && sft > sft0) break;
    if (TH < 1) continue;
    const int64_t PH = TH + (int64_t)(dh_hi - dh_lo), PW = win_w(TW);
    if (PH * PW + (TW - std::min(TW, p.Wg)) > kPatchMaxRows || PW >= 65536) continue;
    const double covered = (double)((p.Hg + TH - 1) / TH) * ((p.Wg + TW - 1) / TW) * 128.0;
    const double util = (double)p.Hg * p.Wg / covered;
    if (util > best_util * 1.02 || (util > best_util * 0.98 && PH * PW < best_P)) {
      best_util = util;
      best_shift = sft;
      best_P = PH * PW;
    }
  }
  const bool window = best_shift >= 0 && bodies_ok;
  int tw_shift = best_shift;
  if (!window) {  // per-tap stages: any shape works, take the least wasteful one
    best_util = -1.0;
    for (int sft = sft0; sft <= 7; ++sft) {
      const int TW = 1 << sft, TH = std::min(128 / TW, p.Hg);
      if (TW > 2 * p.Wg && sft > sft0) break;
      const double covered = (double)((p.Hg + TH - 1) / TH) * ((p.Wg + TW - 1) / TW) * 128.0;
      const double util = (double)p.Hg * p.Wg / covered;
      if (util > best_util) {
        best_util = util;
        tw_shift = sft;
      }
    }
  }
  const int TW = 1 << tw_shift, TH = window ? rows_of(tw_shift) : std::min(128 / TW, p.Hg);
  p.TH = TH;
  p.TW = TW;
  p.tw_shift = tw_shift;
  p.tiles_h = (p.Hg + TH - 1) / TH;
  p.tiles_w = (p.Wg + TW - 1) / TW;
  if (window) {
    const int64_t PH = TH + (int64_t)(dh_hi - dh_lo);
    int64_t PW = win_w(TW);
    // An ODD patch width (the parity classes of a transposed 3x3 convolution: taps 0 / -1, window TW + 1) breaks what the 2-D
    // swizzle key rests on -- "the bank half of LDS row pi * PW + pj is pj & 1" (conv.hip) -- and every second fragment read of
    // those launches is a 2-way bank conflict (scripts/lds_conflicts_conv.py: 1.5 LDS cycles per lane group; PMC: 34-37 % conflict
    // cycles in the upsampler launches, review item 1d).  One unused column makes it even where it fits.
#ifndef VFX_ABL_ODD_PATCH_WIDTH  // (measurement builds keep the odd width)
    if (PH > 1 && (PW & 1) && PH * (PW + 1) + (TW - std::min(TW, p.Wg)) <= kPatchMaxRows) PW += 1;
#endif
    p.per_tap = 0;
    p.PW = (int)PW;
    p.P = (int)(PH * PW);
    p.dh_min = dh_lo;
    p.dw_min = dw_lo;
  } else {
    p.per_tap = 1;
    p.PW = TW;
    p.P = TH * TW;
    p.dh_min = p.dw_min = 0;
  }
}

// Channels per stage: 32, except for an activated source of the 16-bit mode -- an fp16 tensor whose 128-byte patch rows
// hold 64 channels (k_conv, H64).
int stage_channels(const TapConvParams& p, const TapSeg& S) { return (p.hionly && S.src_act) ? 64 : kKC; }

int count_stages(const TapConvParams& p) {  // per phase, for a phased launch
  int n = 0;
  for (int s = 0; s < p.nseg; ++s) n += (p.seg[s].C / stage_channels(p, p.seg[s])) * (p.per_tap ? p.seg[s].ntaps : 1);
  return n;
}

void build_stages(const TapConvParams& p, const float* ones, const float* zeros, ConvStage* out) {
  int k = 0;
  const int64_t tstride = (int64_t)(p.nphase > 1 ? p.cout_phase : p.Cout) * kKC;  // couts of ONE weight tensor
  for (int s = 0; s < p.nseg; ++s) {
    const TapSeg& S = p.seg[s];
    // per-tap launches run tap-major: the patch origin (and with it the kernel's cached pixel offsets)
    // then changes ntaps times per block instead of once per stage
    const int nwin = p.per_tap ? S.ntaps : 1;
    const int kc = stage_channels(p, S);
    const bool f16src = kc == 64;  // activated fp16 tensor: 2 bytes per element, a 64-channel chunk = 128 bytes = 32 floats
    for (int w = 0; w < nwin; ++w)
      for (int ch = 0; ch < S.C / kc; ++ch) {
        ConvStage st{};
        st.src = S.src + ch * kKC;  // 128 bytes per chunk in either form
        st.scale = (S.scale ? S.scale : ones) + (S.scale ? ch * kKC : 0);
        st.shift = (S.shift ? S.shift : zeros) + (S.shift ? ch * kKC : 0);
        st.C = f16src ? S.C / 2 : S.C;  // pixel stride in floats
        st.nbytes = (unsigned)((int64_t)p.B * p.in_img_stride * S.C * (f16src ? 2 : 4) - (int64_t)ch * kKC * 4);
        st.flags = S.src_act ? 1 : 0;
        if (S.src_act) {
          st.scale = ones;
          st.shift = zeros;
        }
        st.slope = S.act == ACT_NONE ? 1.f : S.slope;
        st.tap_stride = (int)tstride;
        if (p.per_tap) {
          st.wt = S.wt + ((int64_t)ch * S.ntaps + w) * tstride;
          st.ntaps = 1;
          st.dh0 = S.dh[w];
          st.dw0 = S.dw[w];
          st.poff[0] = 0;  // tile-sized patch, no shift
        } else {
          st.wt = S.wt + (int64_t)ch * S.ntaps * tstride;
          st.ntaps = S.ntaps;
          st.dh0 = p.dh_min;
          st.dw0 = p.dw_min;
          for (int t = 0; t < S.ntaps; ++t) {  // row offset | column shift << 16 | row shift << 24 (conv.hip, compute())
            const int dpi = S.dh[t] - p.dh_min, dpj = S.dw[t] - p.dw_min;
            VFX_CHECK(dpi < 128 && dpj < 256 && dpi * p.PW + dpj < 65536, "conv: tap offset out of range");
            st.poff[t] = (dpi * p.PW + dpj) | (dpj << 16) | (dpi << 24);
          }
        }
        out[k++] = st;
      }
  }
}

void set_conv1d_geometry(TapConvParams& p, int B, int T, int K, int dil, bool reflect) {
  p.B = B;
  // A dilation too wide for one patch (> 32 samples for k3) is folded: the sequence becomes an image with
  // rows of `dil` samples and the taps become vertical neighbours (TapConvParams, folded geometry).
  const bool fold = !reflect && (K - 1) * dil + 128 > kPatchMaxRows && dil >= 16;
  if (fold) {
    p.Hi = p.Hg = p.Ho = (T + dil - 1) / dil;
    p.Wi = p.Wg = p.Wo = dil;
    p.in_img_stride = p.in_limit = p.out_img_stride = p.out_limit = T;
  } else {
    p.Hi = p.Hg = p.Ho = 1;
    p.Wi = p.Wg = p.Wo = T;
  }
  p.sh = p.sw = 1;
  p.reflect_w = reflect ? 1 : 0;
  TapSeg& S = p.seg[0];
  S.ntaps = K;
  for (int k = 0; k < K; ++k) {
    S.dh[k] = fold ? k - K / 2 : 0;
    S.dw[k] = fold ? 0 : (k - K / 2) * dil;
  }
}

void finish_params(TapConvParams& p) {
  p.total_steps = 0;
  for (int s = 0; s < p.nseg; ++s) {
    VFX_CHECK(p.seg[s].C % stage_channels(p, p.seg[s]) == 0 && p.seg[s].ntaps >= 1 && p.seg[s].ntaps <= kMaxTaps,
              "conv: bad segment %d (C=%d ntaps=%d)", s, p.seg[s].C, p.seg[s].ntaps);
    VFX_CHECK(p.seg[s].C <= kIdentityLen, "conv: segment too wide for the identity tables");
    p.total_steps += p.seg[s].ntaps * (p.seg[s].C / stage_channels(p, p.seg[s]));
  }
  VFX_CHECK(!(p.hionly && p.out_act) || p.Cout % 8 == 0, "conv: an fp16 activated output needs Cout %% 8 == 0");
  VFX_CHECK((int64_t)p.Hi * p.Wi < (int64_t)1 << 31 && (int64_t)p.Ho * p.Wo < (int64_t)1 << 31, "conv: image too large");
  if (p.in_img_stride == 0) p.in_img_stride = p.in_limit = p.Hi * p.Wi;
  if (p.out_img_stride == 0) {
    p.out_img_stride = p.out_limit = p.Ho * p.Wo;
    p.M = p.B * p.Hg * p.Wg;
  } else {
    p.M = p.B * p.out_limit;  // folded 1-D launch: grid == output
  }
  VFX_CHECK((int64_t)p.B * p.Hg * p.Wg < (int64_t)1 << 31, "conv: too many output pixels");
  VFX_CHECK((int64_t)p.B * p.out_img_stride < (int64_t)1 << 31, "conv: too many output pixels");
  VFX_CHECK((int64_t)p.B * p.in_img_stride < (int64_t)1 << 31, "conv: too many input pixels");
  for (int s = 0; s < p.nseg; ++s)  // the kernel addresses a source with 32-bit byte offsets: its bytes as build_stages counts them
    VFX_CHECK((int64_t)p.B * p.in_img_stride * p.seg[s].C * (stage_channels(p, p.seg[s]) == 64 ? 2 : 4) < ((int64_t)1 << 32) - 4096,
              "conv: source tensor of segment %d exceeds 4 GiB", s);
  VFX_CHECK(p.out || p.out_act, "conv: no output");
  VFX_CHECK(!p.residual_act || (p.hionly && !p.residual && p.Cout % 4 == 0 && p.residual_inv_slope >= 1.f),
            "conv: an activated residual needs the 16-bit mode, no raw residual beside it and an invertible LeakyReLU");
  plan_conv(p);
  p.nstages = count_stages(p);
}

// ---------------------------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------------------------
// Debug hooks.  vfx_config.tuning & VFX_TUNE_DEBUG_POISON_ARENA (per handle): the bytes of the arena the plan owns are set to NaN
// patterns before EVERY call (and when the arena grows), so that a kernel reading a workspace buffer nobody wrote shows up whatever
// ran before.  VFX_DEBUG_NAN in the environment, read ONCE per process: after every GEMM-shaped launch the outputs are scanned for
// non-finite values (synchronises; the first hit is reported on stderr).  Plan::run and the entry points do no getenv.
struct DebugSwitches {
  int debug_nan = 0;
  DebugSwitches() {
    if (const char* e = getenv("VFX_DEBUG_NAN")) debug_nan = atoi(e);
  }
};
static const DebugSwitches& debug_switches() {
  static const DebugSwitches s;
  return s;
}
// Called by run_plan before anything of the call is staged in the arena.
static void debug_poison(const vfx_handle* h, const Plan& plan, void* stream) {
  if ((h->cfg.tuning & VFX_TUNE_DEBUG_POISON_ARENA) && plan.bound_base && plan.arena_bytes)
    VFX_HIP(hipMemsetAsync(plan.bound_base, 0xFF, plan.arena_bytes, static_cast<hipStream_t>(stream)));
}

void Plan::run(const RunCtx& ctx) {
  if (debug_switches().debug_nan >= 2 && bound_base && arena_bytes) {
    // whole-arena scan after every op (tiny shapes only)
    for (size_t i = 0; i < ops.size(); ++i) {
      ops[i](ctx);
      const int64_t bad = count_nonfinite(reinterpret_cast<const float*>(bound_base), (int64_t)(arena_bytes / 4), ctx.stream);
      fprintf(stderr, "[vfx debug] after op %zu of %zu: %lld non-finite floats in the arena\n", i, ops.size(), (long long)bad);
    }
    return;
  }
  for (auto& f : ops) f(ctx);
}

static void debug_scan(const Plan* pl, const char* what, size_t idx, const float* rel, int64_t n, int M, int Cout, int K,
                       hipStream_t s) {
  if (!rel) return;
  const float* p = reinterpret_cast<const float*>(pl->bound_base + reinterpret_cast<size_t>(rel) - 1);
  const int64_t bad = count_nonfinite(p, n, s);
  if (bad) fprintf(stderr, "[vfx debug] %s #%zu (M=%d Cout=%d K=%d): %lld of %lld non-finite\n", what, idx, M, Cout, K,
                   (long long)bad, (long long)n);
}

// Algorithmic HBM bytes of a launch (SURVEY.md section 8d accounting: every tensor the launch must read or write,
// once): sources, residual, outputs; weights are L2-resident and not counted.
static double conv_algo_bytes(const TapConvParams& q) {
  const double in_px = (double)q.B * q.in_img_stride, out_px = (double)q.B * q.out_img_stride;
  double b = 0;
  if (q.nphase > 1) {
    b += in_px * q.seg[0].C * ((q.hionly && q.seg[0].src_act) ? 2.0 : 4.0);  // the phases share one source
  } else {
    for (int s2 = 0; s2 < q.nseg; ++s2) b += in_px * q.seg[s2].C * ((q.hionly && q.seg[s2].src_act) ? 2.0 : 4.0);
  }
  if (q.residual) b += out_px * q.Cout * 4.0;
  if (q.residual_act) b += out_px * q.Cout * 2.0;
  if (q.out) b += out_px * (q.out_cmul ? q.out_cmul : q.Cout) * 4.0;
  if (q.out_act) b += out_px * q.Cout * (q.hionly ? 2.0 : 4.0);
  return b;
}
// a ResStack layer's algorithmic bytes are x in + y out = 8 bytes per element and LAYER (a pair
// launch runs two layers).  What the kernel's own design moves on top of that (the fp16 forms xa / ya of the two-form trunk
// of the wide stacks; half of it for a pair, whose intermediate tensor never leaves the CU) is `resblock_design_bytes`.
// On the fp16 trunk of the 16-bit mode (round 4, ResBlockParams::x16) the tensors themselves are 2 bytes per element: x in + y
// out = 4 bytes per element and layer.
static double resblock_algo_bytes(const ResBlockParams& q) {
  const double n = (double)q.B * (q.geo2d ? (double)q.H * q.W : (double)q.T) * q.C;
  if (q.in1) return n * 4.0 + n / q.C * 4.0;  // one input channel in, y out
  if (q.two_src) return n * 12.0;                  // two sources in, y out
  return n * (q.x16 ? 4.0 : 8.0) * (q.dil2 > 0 ? 2.0 : 1.0);
}
static double resblock_design_bytes(const ResBlockParams& q) {
  const double n = (double)q.B * (q.geo2d ? (double)q.H * q.W : (double)q.T) * q.C;
  if (q.in1) return n * 4.0 + n / q.C * 4.0;
  if (q.two_src) return n * 12.0;
  if (q.x16) return n * 2.0 * ((q.x || q.xa ? 1.0 : 0.0) + (q.y ? 1.0 : 0.0) + (q.ya ? 1.0 : 0.0));  // one fp16 tensor in, y and / or ya out
  return n * 8.0 + (q.asrc ? n * 2.0 : 0.0) + (q.ya ? n * 2.0 : 0.0);  // x in, y out (+ the fp16 forms: xa in, ya out)
}

// vfx_profile_*: HIP events around a launch of a profiled call and the record of what ran between them, which `describe` fills
// (flops, bytes and the launch's row of the VFX_PROFILE_DUMP table).  An unprofiled call just launches.
template <class Launch, class Describe>
static void profiled(const RunCtx& c, Launch launch, Describe describe) {
  const bool on = c.prof && c.prof->enabled;
  LaunchRecord r{};
  if (on) {
    VFX_HIP(hipEventCreate(&r.begin));
    VFX_HIP(hipEventCreate(&r.end));
    VFX_HIP(hipEventRecord(r.begin, c.stream));
  }
  launch();
  if (on) {
    VFX_HIP(hipEventRecord(r.end, c.stream));
    describe(r);
    c.prof->launches.push_back(r);
  }
}

void PlanBuilder::add_conv(TapConvParams p) {
  p.split = h->cfg.precision != 0;
  p.tuning = h->cfg.tuning;
  p.short_clip = short_clip;
  finish_params(p);
  p.ksplit = (p.lens || no_splitk) ? 1 : choose_ksplit(p);  // (a launch with per-clip lengths skips the tiles past a clip's end)
  size_t ws_off = ~size_t(0);
  if (p.ksplit > 1) {  // the partial tiles live in the arena for the duration of this op
    ws_off = alloc_f((int64_t)p.ksplit * p.B * p.out_img_stride * p.Cout);
    p.ws = const_cast<float*>(rel_ptr(ws_off));
  } else {
    p.ksplit = 0;
  }
  // TapConvParams::w64: the launch runs on k_conv_w64 where the plan asked for it and the kernel has the shape.  Such a launch keeps
  // k_conv's tile geometry and gets its stage table at bind time all the same -- the kernel reads neither (host work per plan, a few
  // microseconds); conv_w64_ok and the profile row read the geometry fields finish_params filled.
  plan_conv_w64(p);
  const size_t idx = plan->host_params.size();
  plan->host_params.push_back(p);
  plan->conv_flops += conv_flops(p);
  plan->n_conv += 1;
  Plan* pl = plan;
  plan->ops.push_back([pl, idx](const RunCtx& c) {
    const TapConvParams& hp = pl->host_params[idx];
    profiled(c, [&] {
      launch_conv(hp, pl->dev_params + idx, c.stream);
      if (hp.ksplit > 1) launch_splitk_reduce(pl->abs_params[idx], c.stream);  // the same stream: ordered behind the partial tiles
    }, [&](LaunchRecord& r) {
      r.flops = conv_flops(hp);
      r.bytes = r.design_bytes = conv_algo_bytes(hp);
      if (hp.up16) {  // a ConvTranspose1d of the 16-bit mode on its own kernel (upsample16.hip)
        snprintf(r.kernel, sizeof(r.kernel), "k_up16<%d; 128> f16", hp.seg[0].C / 64);
      } else if (hp.w64.on) {  // a ResStack convolution of the 16-bit mode on the wide-wave kernel (conv_w64.hip)
        snprintf(r.kernel, sizeof(r.kernel), "k_conv_w64<%d> f16", hp.seg[0].C / 64);
      } else {
        bool elu = false;
        for (int s2 = 0; s2 < hp.nseg; ++s2) elu = elu || hp.seg[s2].act == ACT_ELU;
        snprintf(r.kernel, sizeof(r.kernel), "k_conv<%d; %s; %s>%s", conv_block_n(hp), elu ? "true" : "false", hp.split ? "true" : "false",
                 hp.hionly ? " f16" : "");
      }
      r.M = hp.M;
      r.Cout = hp.Cout;
      for (int s2 = 0; s2 < hp.nseg; ++s2) r.K += hp.seg[s2].ntaps * hp.seg[s2].C;
      r.nseg = hp.nseg;
      r.ntaps0 = hp.seg[0].ntaps;
      r.C0 = hp.seg[0].C;
      r.Wi = hp.Wi;
      r.sw = hp.sw;
    });
    if (debug_switches().debug_nan) {
      const TapConvParams& q = pl->host_params[idx];
      int K = 0;
      for (int s2 = 0; s2 < q.nseg; ++s2) K += q.seg[s2].ntaps * q.seg[s2].C;
      const int64_t n = (int64_t)q.B * q.out_img_stride * (q.out_cmul ? q.out_cmul : q.Cout);
      debug_scan(pl, "conv out", idx, q.out, n, q.M, q.Cout, K, c.stream);
      debug_scan(pl, "conv out_act", idx, q.out_act, n, q.M, q.Cout, K, c.stream);
    }
  });
  if (ws_off != ~size_t(0)) free(ws_off);
}

void PlanBuilder::add_conv_phased(TapConvParams p, const std::vector<TapSeg>& phases) {
  VFX_CHECK(p.nseg == 1 && !phases.empty() && p.Cout % (int)phases.size() == 0, "phased conv: bad arguments");
  p.nphase = (int)phases.size();
  p.cout_phase = p.Cout / p.nphase;
  VFX_CHECK(p.cout_phase % 32 == 0, "phased conv: %d couts per phase", p.cout_phase);
  VFX_CHECK(!p.out_cmul || (p.out_cmul == p.cout_phase && p.nphase == (p.phase_rows ? 4 : 2) && p.sw == 2 && p.ow0 == 0 && !p.residual &&
                            !p.residual_act && !p.out_act && p.out && !p.bias),
            "phased conv: bad odd-width launch");
  VFX_CHECK(!p.phase_rows || (p.out_cmul && p.sh == 2 && p.oh0 == 0 && p.Wo >= 2), "phased conv: bad row-phased launch");
  const size_t idx = plan->host_params.size();
  plan->phase_segs[idx] = phases;
  add_conv(p);
  TapConvParams& hp = plan->host_params[idx];
  VFX_CHECK(!hp.per_tap, "phased conv: the union of the phases' taps does not fit one patch");
  // algorithmic work: every phase multiplies by its own taps only
  double k = 0;
  for (auto& S : phases) k += (double)S.ntaps * S.C;
  const double fl = 2.0 * (double)hp.M * hp.cout_phase * k;
  plan->conv_flops += fl - conv_flops(hp);
  hp.flops_override = fl;
  hp.up16 = upsample16_selected(hp, phases) ? 1 : 0;
}

void PlanBuilder::add_resblock(ResBlockParams p) {
  p.tuning = h->cfg.tuning;
  if (p.geo2d) plan_block2d(p);
  else plan_resblock(p);
  const size_t idx = plan->host_rb.size();
  plan->host_rb.push_back(p);
  plan->conv_flops += resblock_flops(p);
  plan->n_conv += 1;
  Plan* pl = plan;
  plan->ops.push_back([pl, idx](const RunCtx& c) {
    const ResBlockParams& hp = pl->host_rb[idx];
    profiled(c, [&] { launch_resblock(hp, pl->dev_rb + idx, c.stream); }, [&](LaunchRecord& r) {
      r.flops = resblock_flops(hp);
      r.bytes = resblock_algo_bytes(hp);
      r.design_bytes = resblock_design_bytes(hp);
      const bool pair = hp.dil2 > 0, persistent2d = block2d32_ok(hp);
      snprintf(r.kernel, sizeof(r.kernel), "%s<%d; %d>%s", pair ? "k_resblock_pair" : (persistent2d ? "k_block2d" : "k_resblock"), hp.C,
               resblock_block_waves(hp) /* waves per block */, hp.hionly ? " f16" : "");
      // a fused ResStack layer in the columns of a convolution: M = B * T, Cout = C0 = C, K = nseg = sw = 0, Wi = the dilation and
      // ntaps0 = the taps it fuses (6; pairs: four convolutions, 12; 18: the persistent 2-D block)
      r.M = hp.B * hp.T;
      r.Cout = r.C0 = hp.C;
      r.ntaps0 = pair ? 12 : (persistent2d ? 18 : 6);
      r.Wi = hp.dil;
    });
    if (debug_switches().debug_nan && hp.y && !hp.x16)
      debug_scan(pl, "resblock y", idx, hp.y, (int64_t)hp.B * hp.T * hp.C, hp.B * hp.T, hp.C, 6 * hp.C, c.stream);
  });
}

char* GrowBuffer::ensure(vfx_handle* h, size_t need, size_t slack_div, const char* pinned_msg) {
  if (need <= bytes) return p;
  if (pinned_msg)
    for (auto& kv : h->plans) VFX_CHECK(!kv.second->pinned, pinned_msg, bytes, need, kv.first.c_str());
  VFX_HIP(hipDeviceSynchronize());   // the previous buffer may still be read by launches in flight
  const bool arena = this == &h->arena;
  if (arena) h->retired.clear();  // (evicted plans: their parameter blocks go now, the device is idle)
  if (p) VFX_HIP(hipFree(p));
  p = nullptr;
  bytes = 0;
  const size_t want = need + (slack_div ? need / slack_div : 0);
  void* q = nullptr;
  VFX_HIP(hipMalloc(&q, want));
  // Debug aid (tests): a freshly grown arena is filled with NaN patterns, so that a kernel reading a
  // workspace buffer before anything wrote it shows up as NaN instead of silently using stale values.
  if (arena && (h->cfg.tuning & VFX_TUNE_DEBUG_POISON_ARENA)) VFX_HIP(hipMemset(q, 0xFF, want));
  p = static_cast<char*>(q);
  bytes = want;
  return p;
}

char* StagedUpload::stage(vfx_handle* h, size_t bytes) {
  if (pending) VFX_HIP(hipEventSynchronize(copied));
  pending = false;
  dev.ensure(h, bytes, 0);
  if (bytes > host_bytes) {
    if (host) VFX_HIP(hipHostFree(host));
    host = nullptr;
    host_bytes = 0;
    void* q = nullptr;
    VFX_HIP(hipHostMalloc(&q, bytes, hipHostMallocDefault));
    host = static_cast<char*>(q);
    host_bytes = bytes;
  }
  return host;
}

char* StagedUpload::upload(size_t bytes, hipStream_t s) {
  if (!copied) VFX_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
  VFX_HIP(hipMemcpyAsync(dev.p, host, bytes, hipMemcpyHostToDevice, s));
  VFX_HIP(hipEventRecord(copied, s));
  pending = true;
  return dev.p;
}

// Rebase the plan's arena-relative pointers on the (possibly re-allocated) arena and upload
// the parameter blocks.
void bind_plan(vfx_handle* h, Plan& plan) {
  // A hipGraph captured from a plan (Plan::pinned) replays kernels whose parameter blocks hold ABSOLUTE pointers into the arena
  // as it was at capture time.  Growing the arena frees that memory: the next replay would read and write freed memory with no
  // error.  So a handle with a captured plan refuses to grow; the caller reserves the largest shape first (vfx_reserve), then
  // captures.  (Before the first allocation there is nothing to point into.)
  char* base = h->arena.ensure(h, plan.arena_bytes, 16, !h->arena.p ? nullptr :
      "the workspace arena would have to grow from %zu to %zu bytes, but a hipGraph was captured from plan '%s' "
      "and replays kernels that point into the current arena: vfx_reserve() the largest (model, B, T) BEFORE capturing, "
      "or destroy the graph(s) and call vfx_unpin_plans(); if this call was itself being captured, that capture has failed");
  if (plan.bound_base == base && (plan.dev_params || plan.dev_rb || (plan.host_params.empty() && plan.host_rb.empty()))) return;
  std::vector<TapConvParams> abs = plan.host_params;
  auto rebase = [&](const float* rel) -> const float* {
    return reinterpret_cast<const float*>(base + reinterpret_cast<size_t>(rel) - 1);
  };
  size_t total_stages = 0;
  for (auto& p : abs) total_stages += (size_t)p.nstages * std::max(p.nphase, 1);
  if (!plan.dev_stages && total_stages)
    plan.dev_stages = static_cast<ConvStage*>(plan.blob.alloc(total_stages * sizeof(ConvStage)));
  std::vector<ConvStage> stages(total_stages);
  size_t so = 0;
  for (auto& p : abs) {
    for (int s = 0; s < p.nseg; ++s) p.seg[s].src = rebase(p.seg[s].src);
    if (p.residual) p.residual = rebase(p.residual);
    if (p.residual_act) p.residual_act = rebase(p.residual_act);
    if (p.out) p.out = const_cast<float*>(rebase(p.out));
    if (p.out_act) p.out_act = const_cast<float*>(rebase(p.out_act));
    if (p.ws) p.ws = const_cast<float*>(rebase(p.ws));
    p.flags = h->d_flags;
    const size_t pidx = &p - abs.data();
    if (p.nphase > 1) {  // one stage table per phase, built from that phase's segment on the common patch geometry
      const std::vector<TapSeg>& segs = plan.phase_segs.at(pidx);
      for (int r = 0; r < p.nphase; ++r) {
        TapConvParams q = p;
        q.seg[0] = segs[r];
        q.seg[0].src = rebase(q.seg[0].src);
        build_stages(q, h->d_ones, h->d_zeros, stages.data() + so + (size_t)r * p.nstages);
      }
    } else {
      build_stages(p, h->d_ones, h->d_zeros, stages.data() + so);
    }
    p.stages = plan.dev_stages + so;
    so += (size_t)p.nstages * std::max(p.nphase, 1);
  }
  if (total_stages)
    VFX_HIP(hipMemcpy(plan.dev_stages, stages.data(), total_stages * sizeof(ConvStage), hipMemcpyHostToDevice));
  if (!plan.dev_params && !abs.empty())
    plan.dev_params = static_cast<TapConvParams*>(plan.blob.alloc(abs.size() * sizeof(TapConvParams)));
  if (!abs.empty())
    VFX_HIP(hipMemcpy(plan.dev_params, abs.data(), abs.size() * sizeof(TapConvParams), hipMemcpyHostToDevice));
  plan.abs_params = abs;  // host copy with absolute pointers (split-K reduce launches)
  if (!plan.host_rb.empty()) {
    std::vector<ResBlockParams> rb = plan.host_rb;
    for (auto& q : rb) {
      if (q.x) q.x = rebase(q.x);
      if (q.x2) q.x2 = rebase(q.x2);
      if (q.y) q.y = const_cast<float*>(rebase(q.y));
      if (q.xa) q.xa = rebase(q.xa);
      if (q.ya) q.ya = const_cast<float*>(rebase(q.ya));
      q.flags = h->d_flags;
    }
    if (!plan.dev_rb) plan.dev_rb = static_cast<ResBlockParams*>(plan.blob.alloc(rb.size() * sizeof(ResBlockParams)));
    VFX_HIP(hipMemcpy(plan.dev_rb, rb.data(), rb.size() * sizeof(ResBlockParams), hipMemcpyHostToDevice));
  }
  plan.bound_base = base;
}

// ---------------------------------------------------------------------------------------------
// plan cache
// ---------------------------------------------------------------------------------------------
static std::shared_ptr<Plan> get_plan(vfx_handle* h, const std::string& key,
                                      const std::function<void(PlanBuilder&)>& build, void* stream) {
  auto it = h->plans.find(key);
  std::shared_ptr<Plan> plan;
  if (it == h->plans.end()) {
    plan = std::make_shared<Plan>();
    PlanBuilder pb{h, plan.get(), {}};
    build(pb);
    plan->arena_bytes = pb.arena.high;
    // bounded cache: drop the least recently used plan(s) first (their parameter blocks are hipFree'd, which waits
    // for the device: nothing in flight still reads them).  Plans a hipGraph was captured from are never dropped: the
    // graph's kernel nodes keep the plan's device parameter blocks as arguments (the cache then grows past the bound).
    while (h->plans.size() >= kMaxCachedPlans) {
      auto victim = h->plans.end();
      for (auto i = h->plans.begin(); i != h->plans.end(); ++i)
        if (!i->second->pinned && (victim == h->plans.end() || i->second->last_use < victim->second->last_use)) victim = i;
      if (victim == h->plans.end()) break;
      // the victim's parameter blocks are hipFree'd when the Plan dies, and hipFree waits for the whole device: retire it instead and
      // let the plans go in batches (every 64 evictions, when the arena grows -- both wait for the device anyway -- and at
      // vfx_destroy), so that a test set with more distinct shapes than the cache holds does not stall the GPU once per call
      h->retired.push_back(victim->second);
      h->plans.erase(victim);
      if (h->retired.size() >= 64) h->retired.clear();
    }
    h->plans[key] = plan;
  } else {
    plan = it->second;
  }
  bool capturing = false;
  if (stream) {  // the legacy (NULL) stream cannot be captured
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    capturing = hipStreamIsCapturing(static_cast<hipStream_t>(stream), &st) == hipSuccess && st == hipStreamCaptureStatusActive;
  }
  plan->last_use = ++h->plan_tick;
  // bind first, pin afterwards: when the arena would have to grow under a capture (or under an older pinned plan)
  // GrowBuffer::ensure throws, the capture fails in the caller -- and a plan no graph was captured from must not stay pinned, it
  // would refuse every later growth until somebody finds vfx_unpin_plans()
  bind_plan(h, *plan);
  if (capturing) plan->pinned = true;
  return plan;
}

std::string key_of(const char* tag, int B, int T, int x) {
  char buf[96];
  snprintf(buf, sizeof(buf), "%s:%d:%d:%d", tag, B, T, x);
  return buf;
}

std::shared_ptr<Plan> run_plan(vfx_handle* h, const std::string& key, void* stream, std::initializer_list<const float*> ext,
                               const std::function<void(PlanBuilder&)>& build, const std::function<void(Plan&)>& before) {
  auto plan = get_plan(h, key, build, stream);
  debug_poison(h, *plan, stream);
  if (before) before(*plan);
  RunCtx ctx{static_cast<hipStream_t>(stream), {}, h->d_flags, &h->prof};
  std::transform(ext.begin(), ext.end(), ctx.ext, [](const float* p) { return const_cast<float*>(p); });
  plan->run(ctx);
  return plan;
}

}  // namespace vfx
