// ops_debug.cpp -- libvfx_test.so: kernel-level C entry points used by the parity tests (include/vfx_test.h).
// They pack PyTorch-layout weights on the fly, run one kernel family of libvfx.so and synchronise; vfx_op_voc_* and vfx_op_unet_piece
// run single launches of the vocoder and ResUNet plans through the plans' own builder functions (vocoder.cpp, resunet.cpp) -- no
// launch parameters of those plans are restated here (vfx_op_resblock / vfx_op_resblock_pair, the older entry points of the fused ResStack
// layers, fill theirs by hand; vfx_op_voc_resblock is the plan's form).  Not part of the product library: built into its own shared object that
// resolves the internals it uses from libvfx.so.
#include <cmath>
#include <cstring>

#include "vfx_internal.h"
#include "vfx_test.h"

using namespace vfx;

namespace {
struct Scratch {
  DeviceBlob blob;
};

void fill_seg(TapSeg& S, const float* x, int Cin, const float* scale, const float* shift, int act, float slope,
              DeviceBlob& blob) {
  S.src = x;
  S.C = Cin;
  std::vector<float> one(Cin, 1.f), zero(Cin, 0.f);
  S.scale = blob.upload(scale ? scale : one.data(), Cin);
  S.shift = blob.upload(shift ? shift : zero.data(), Cin);
  S.act = act;
  S.slope = slope;
}

void run_one(vfx_handle* h, TapConvParams& p, DeviceBlob& blob, hipStream_t s) {
  p.split = h->cfg.precision != 0;
  p.hionly = h->cfg.precision == 2;
  p.flags = h->d_flags;
  p.tuning = h->cfg.tuning;
  finish_params(p);
  std::vector<ConvStage> st(p.nstages);
  build_stages(p, h->d_ones, h->d_zeros, st.data());
  ConvStage* ds = static_cast<ConvStage*>(blob.alloc(st.size() * sizeof(ConvStage)));
  VFX_HIP(hipMemcpy(ds, st.data(), st.size() * sizeof(ConvStage), hipMemcpyHostToDevice));
  p.stages = ds;
  p.ksplit = choose_ksplit(p);
  if (p.ksplit > 1) p.ws = static_cast<float*>(blob.alloc((size_t)p.ksplit * p.B * p.out_img_stride * p.Cout * sizeof(float)));
  else p.ksplit = 0;
  TapConvParams* d = static_cast<TapConvParams*>(blob.alloc(sizeof(TapConvParams)));
  VFX_HIP(hipMemcpy(d, &p, sizeof(p), hipMemcpyHostToDevice));
  launch_conv(p, d, s);
  if (p.ksplit > 1) launch_splitk_reduce(p, s);
}

// A phased launch (TapConvParams::nphase: the column classes of a transposed convolution's row class as ONE launch), set up the way
// PlanBuilder::add_conv_phased / bind_plan do it: p.seg[0] = the union window, one stage table per phase.
void run_phased(vfx_handle* h, TapConvParams& p, const std::vector<TapSeg>& phases, DeviceBlob& blob, hipStream_t s) {
  p.split = h->cfg.precision != 0;
  p.hionly = h->cfg.precision == 2;
  p.flags = h->d_flags;
  p.tuning = h->cfg.tuning;
  p.nphase = (int)phases.size();
  p.cout_phase = p.Cout / p.nphase;
  finish_params(p);
  VFX_CHECK(!p.per_tap, "phased conv: the union of the phases' taps does not fit one patch");
  std::vector<ConvStage> st((size_t)p.nstages * p.nphase);
  for (int r = 0; r < p.nphase; ++r) {
    TapConvParams q = p;
    q.seg[0] = phases[r];
    build_stages(q, h->d_ones, h->d_zeros, st.data() + (size_t)r * p.nstages);
  }
  ConvStage* ds = static_cast<ConvStage*>(blob.alloc(st.size() * sizeof(ConvStage)));
  VFX_HIP(hipMemcpy(ds, st.data(), st.size() * sizeof(ConvStage), hipMemcpyHostToDevice));
  p.stages = ds;
  p.ksplit = 0;
  TapConvParams* d = static_cast<TapConvParams*>(blob.alloc(sizeof(TapConvParams)));
  VFX_HIP(hipMemcpy(d, &p, sizeof(p), hipMemcpyHostToDevice));
  launch_conv(p, d, s);
}
}  // namespace

extern "C" int vfx_op_conv(vfx_handle* h, const float* x, int B, int H, int W, int Cin, const float* weight, int Cout,
                           int kh, int kw, int dil_w, int reflect_w, const float* scale, const float* shift, int act,
                           float slope, const float* bias, const float* residual, float* y, void* stream) {
  try {
    VFX_CHECK(h && x && weight && y, "NULL argument");
    VFX_CHECK(kh * kw <= kMaxTaps, "vfx_op_conv: at most %d taps", kMaxTaps);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    std::vector<std::pair<int, int>> taps;
    TapConvParams p{};
    TapSeg& S = p.seg[0];
    for (int a = 0; a < kh; ++a)
      for (int b = 0; b < kw; ++b) {
        S.dh[taps.size()] = a - kh / 2;
        S.dw[taps.size()] = (b - kw / 2) * dil_w;
        taps.push_back({a, b});
      }
    S.ntaps = (int)taps.size();
    fill_seg(S, x, Cin, scale, shift, act, slope, sc.blob);
    S.wt = sc.blob.upload(pack_conv(weight, Cout, Cin, kh, kw, 0, Cin, taps, h->cfg.precision == 2 ? 2 : (h->cfg.precision != 0)));
    p.nseg = 1;
    p.B = B;
    p.Hi = p.Hg = p.Ho = H;
    p.Wi = p.Wg = p.Wo = W;
    p.sh = p.sw = 1;
    p.reflect_w = reflect_w;
    if (H == 1 && kh == 1 && !reflect_w) set_conv1d_geometry(p, B, W, kw, dil_w, false);  // folds wide dilations
    p.Cout = Cout;
    p.bias = bias ? sc.blob.upload(bias, Cout) : nullptr;
    p.residual = residual;
    p.out = y;
    p.act_slope = 1.f;
    run_one(h, p, sc.blob, s);
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// The activated fp16 output of a fused layer must be fp16(LeakyReLU(y)) exactly: checked inside the debug entry points so that a
// test sees a mismatch as an error of the call.
static void check_activated_output(const float* y, const float* dya, size_t n, float slope, hipStream_t s) {
  VFX_HIP(hipStreamSynchronize(s));
  std::vector<float> hy(n);
  std::vector<_Float16> hya(n);
  VFX_HIP(hipMemcpy(hy.data(), y, n * sizeof(float), hipMemcpyDeviceToHost));
  VFX_HIP(hipMemcpy(hya.data(), dya, n * sizeof(_Float16), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    const float v = hy[i] > 0.f ? hy[i] : hy[i] * slope;
    const _Float16 e = (_Float16)std::min(std::max(v, -65504.f), 65504.f);
    VFX_CHECK((float)e == (float)hya[i], "activated output differs from fp16(LeakyReLU(y)) at element %zu (%g vs %g)", i,
              (double)(float)hya[i], (double)(float)e);
  }
}

// ---- fp16 trunk of the 16-bit mode (ResBlockParams::x16): the debug entry points keep their fp32 interface and convert ----------
static bool handle_trunk_f16(const vfx_handle* h) { return h->cfg.precision == 2 && !(h->cfg.tuning & VFX_TUNE_F32_TRUNK); }

// device fp32 tensor -> a device fp16 tensor holding fp16(f(x)), f = LeakyReLU(slope) (slope = 1: the raw trunk)
static float* to_device_f16(DeviceBlob& blob, const float* dx, size_t n, float slope) {
  std::vector<float> hx(n);
  VFX_HIP(hipMemcpy(hx.data(), dx, n * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<_Float16> hh(n);
  for (size_t i = 0; i < n; ++i) {
    const float v = hx[i] > 0.f ? hx[i] : hx[i] * slope;
    hh[i] = (_Float16)std::min(std::max(v, -65504.f), 65504.f);
  }
  void* d = blob.alloc(n * sizeof(_Float16));
  VFX_HIP(hipMemcpy(d, hh.data(), n * sizeof(_Float16), hipMemcpyHostToDevice));
  return static_cast<float*>(d);
}
static std::vector<_Float16> download_f16(const float* d, size_t n) {
  std::vector<_Float16> hh(n);
  VFX_HIP(hipMemcpy(hh.data(), d, n * sizeof(_Float16), hipMemcpyDeviceToHost));
  return hh;
}
// device fp16 tensor holding LeakyReLU(y, slope) (slope = 1: y itself) -> the caller's device fp32 tensor y
static void from_device_f16(const float* d16, float* dy, size_t n, float slope) {
  const std::vector<_Float16> hh = download_f16(d16, n);
  std::vector<float> hy(n);
  for (size_t i = 0; i < n; ++i) hy[i] = (float)hh[i] >= 0.f ? (float)hh[i] : (float)hh[i] / slope;
  VFX_HIP(hipMemcpy(dy, hy.data(), n * sizeof(float), hipMemcpyHostToDevice));
}
// Runs a planned layer (or pair) of the raw fp16 trunk twice -- y16 + ya, then ya alone (the last layer in front of an upsampler
// stores no raw output) -- checks that ya is the same bit pattern both times and that it fits y16, and returns y16 widened in the
// caller's fp32 tensor.  The kernels (resblock_rw.hip, resblock_r128.hip) round BOTH outputs from the same unrounded fp32 sum s:
// y16 = fp16(s), ya = fp16(fl32(max(s, s * slope))).  So where y16 >= 0, ya is y16 itself (0 < slope <= 1: the maximum is s); where
// y16 < 0, s lies within half an fp16 ulp hu(y16) of y16 and ya within half an fp16 ulp of slope * s:
//   |ya - slope * y16| <= slope * hu(y16) + hu(w) + 2^-24 w,  w = slope * (|y16| + hu(y16)),  hu(a) = 2^(max(ilogb(a), -14) - 11)
// -- at most |slope * y16| / 1024 + 2^-24, half of the 1 / 512 this check allowed before.
static void run_raw_f16_trunk(ResBlockParams rp, float* y_out, size_t n, float slope, DeviceBlob& blob, hipStream_t s) {
  float* y16 = static_cast<float*>(blob.alloc(n * sizeof(_Float16)));
  float* ya_a = static_cast<float*>(blob.alloc(n * sizeof(_Float16)));
  float* ya_b = static_cast<float*>(blob.alloc(n * sizeof(_Float16)));
  rp.x16 = 1;
  rp.act_slope = slope;
  for (int pass = 0; pass < 2; ++pass) {
    rp.y = pass == 0 ? y16 : nullptr;
    rp.ya = pass == 0 ? ya_a : ya_b;
    plan_resblock(rp);
    ResBlockParams* d = static_cast<ResBlockParams*>(blob.alloc(sizeof(ResBlockParams)));
    VFX_HIP(hipMemcpy(d, &rp, sizeof(rp), hipMemcpyHostToDevice));
    launch_resblock(rp, d, s);
  }
  VFX_HIP(hipStreamSynchronize(s));
  const std::vector<_Float16> hy = download_f16(y16, n), ha = download_f16(ya_a, n), hb = download_f16(ya_b, n);
  for (size_t i = 0; i < n; ++i) {
    VFX_CHECK(__builtin_bit_cast(unsigned short, ha[i]) == __builtin_bit_cast(unsigned short, hb[i]),
              "fp16 trunk: ya differs between the launch with and without the raw output at element %zu", i);
    const double yv = (double)(float)hy[i], av = (double)(float)ha[i];
    if (yv >= 0.0) {
      VFX_CHECK(av == yv, "fp16 trunk: ya is not y at element %zu, where y >= 0 (%g vs %g)", i, av, yv);
    } else {
      auto hu = [](double a) { return std::ldexp(1.0, std::max(std::ilogb(a), -14) - 11); };
      const double w = (double)slope * (-yv + hu(yv));
      VFX_CHECK(std::fabs(av - (double)slope * yv) <= (double)slope * hu(yv) + hu(w) + std::ldexp(w, -24),
                "fp16 trunk: ya is not within half an fp16 ulp of LeakyReLU(s) at element %zu (%g vs y = %g)", i, av, yv);
    }
  }
  from_device_f16(y16, y_out, n, 1.f);
}

// One ResStack layer y = x + conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 on (B, T, C) tensors; weights in PyTorch
// Conv1d layout (C, C, 3) on the HOST.  fused != 0: k_resblock (C = 64 / 128, split-bf16 mode only);
// fused == 0: two k_conv launches with the ACTIVATED intermediate tensor (any C multiple of 32), which is what
// the plans use for the wide stacks -- this path also exercises the folded geometry for dil > 32.
extern "C" int vfx_op_resblock(vfx_handle* h, const float* x, int B, int T, int C, const float* w1, const float* b1,
                               const float* w2, const float* b2, int dil, float slope, int fused, float* y, void* stream) {
  try {
    VFX_CHECK(h && x && w1 && b1 && w2 && b2 && y, "NULL argument");
    VFX_CHECK(C % kKC == 0 && B > 0 && T > 0 && dil >= 1, "vfx_op_resblock: bad shape");
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const bool split = h->cfg.precision != 0;
    std::vector<std::pair<int, int>> taps = {{0, 0}, {0, 1}, {0, 2}};
    const int pmode = h->cfg.precision == 2 ? 2 : (int)split;
    // two-launch form, 16-bit mode: h travels as an activated fp16 tensor (64-channel stages) when C allows it
    const bool h_f16 = !fused && h->cfg.precision == 2 && C % 64 == 0;
    const bool h_act = !(h->cfg.precision == 2 && !h_f16);
    float* dw1 = sc.blob.upload(pack_conv(w1, C, C, 1, 3, 0, C, taps, pmode));
    float* dw2 = sc.blob.upload(pack_conv(w2, C, C, 1, 3, 0, C, taps, h_f16 ? 3 : pmode));
    float* db1 = sc.blob.upload(b1, C);
    float* db2 = sc.blob.upload(b2, C);
    const size_t nel = (size_t)B * T * C;
    const bool t16 = handle_trunk_f16(h);
    if (fused && h->cfg.precision == 2 && resblock_w64_supported(C)) {
      // wide fused layer of the 16-bit mode: conv1 reads xa = fp16(LeakyReLU(x)), built here on the host.  Two-form trunk
      // (VFX_TUNE_F32_TRUNK): x / y raw fp32 beside xa / ya; fp16 trunk: xa -> ya alone, y = LeakyReLU^-1(ya) for the caller.
      float* dxa = to_device_f16(sc.blob, x, nel, slope);
      float* dya = static_cast<float*>(sc.blob.alloc(nel * sizeof(_Float16)));
      ResBlockParams rp{};
      rp.asrc = 1;
      rp.x16 = t16 ? 1 : 0;
      rp.tuning = h->cfg.tuning;
      rp.x = t16 ? nullptr : x;
      rp.xa = dxa;
      rp.y = t16 ? nullptr : y;
      rp.ya = dya;
      rp.act_slope = slope;
      rp.w1 = sc.blob.upload(pack_conv(w1, C, C, 1, 3, 0, C, taps, 3));
      rp.w2 = sc.blob.upload(pack_conv(w2, C, C, 1, 3, 0, C, taps, 3));
      rp.b1 = db1;
      rp.b2 = db2;
      rp.slope = slope;
      rp.B = B;
      rp.T = T;
      rp.C = C;
      rp.hionly = 1;
      rp.flags = h->d_flags;
      rp.dil = dil;
      plan_resblock(rp);
      ResBlockParams* d = static_cast<ResBlockParams*>(sc.blob.alloc(sizeof(ResBlockParams)));
      VFX_HIP(hipMemcpy(d, &rp, sizeof(rp), hipMemcpyHostToDevice));
      launch_resblock(rp, d, s);
      if (t16) {
        VFX_HIP(hipStreamSynchronize(s));
        from_device_f16(dya, y, nel, slope);
      } else {
        check_activated_output(y, dya, nel, slope, s);
      }
    } else if (fused) {
      VFX_CHECK(split && resblock_supported(C), "vfx_op_resblock: the fused kernel needs precision 1 or 2 and C = 64 or 128 (precision 2: also 256)");
      ResBlockParams rp{};
      rp.x = x;
      rp.y = y;
      rp.w1 = dw1;
      rp.w2 = dw2;
      rp.b1 = db1;
      rp.b2 = db2;
      rp.slope = slope;
      rp.B = B;
      rp.T = T;
      rp.C = C;
      rp.hionly = h->cfg.precision == 2;
      rp.tuning = h->cfg.tuning;
      rp.flags = h->d_flags;
      rp.dil = dil;
      // fp16 trunk: wherever the plan would run this layer on it (vocoder.cpp stack_trunk_f16: resblock_r128, resblock_rw)
      if (rp.hionly && t16 && (C == 128 || (C == 64 && resblock_rw_tile(h->cfg.tuning) != 0))) {
        rp.x = to_device_f16(sc.blob, x, nel, 1.f);
        run_raw_f16_trunk(rp, y, nel, slope, sc.blob, s);
      } else {
        float* dya = nullptr;
        if (rp.hionly) {  // 16-bit mode: also the activated fp16 form a last layer writes for the upsampler behind it
          dya = static_cast<float*>(sc.blob.alloc(nel * sizeof(_Float16)));
          rp.ya = dya;
          rp.act_slope = slope;
        }
        plan_resblock(rp);
        ResBlockParams* d = static_cast<ResBlockParams*>(sc.blob.alloc(sizeof(ResBlockParams)));
        VFX_HIP(hipMemcpy(d, &rp, sizeof(rp), hipMemcpyHostToDevice));
        launch_resblock(rp, d, s);
        if (dya) check_activated_output(y, dya, nel, slope, s);
      }
    } else {
      float* hbuf = static_cast<float*>(sc.blob.alloc((size_t)B * T * C * sizeof(float)));
      TapConvParams p1{};
      set_conv1d_geometry(p1, B, T, 3, dil, false);
      p1.Cout = C;
      p1.nseg = 1;
      fill_seg(p1.seg[0], x, C, nullptr, nullptr, ACT_LEAKY, slope, sc.blob);
      p1.seg[0].wt = dw1;
      p1.bias = db1;
      if (h_act) {
        p1.out_act = hbuf;  // activated with conv2's prologue
        p1.act_slope = slope;
      } else {
        p1.out = hbuf;      // raw: conv2 applies the LeakyReLU itself
        p1.act_slope = 1.f;
      }
      run_one(h, p1, sc.blob, s);
      TapConvParams p2{};
      set_conv1d_geometry(p2, B, T, 3, 1, false);
      p2.Cout = C;
      p2.nseg = 1;
      fill_seg(p2.seg[0], hbuf, C, nullptr, nullptr, h_act ? ACT_NONE : ACT_LEAKY, h_act ? 1.f : slope, sc.blob);
      p2.seg[0].src_act = h_act ? 1 : 0;
      p2.seg[0].wt = dw2;
      p2.bias = db2;
      p2.residual = x;
      p2.out = y;
      p2.act_slope = 1.f;
      run_one(h, p2, sc.blob, s);
    }
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// Host-only: the tile geometry plan_resblock() gives one fused ResStack layer (or layer pair, dil2 > 0) of `C` channels over
// sequences of `T` positions in precision mode `precision` -- so that the CPU test suite can check that the tiles of every
// kernel family (1-D, folded, pairs; 128- and 256-position tiles) write each output position exactly once.
// out[12] = fold, TH, W1, TWo, tiles_h, tiles_w, PW, P, tile_m, rw, patch_rows, asrc.  Needs no GPU and no handle.
extern "C" int vfx_plan_resblock_geometry_tuned(int C, int T, int dil, int dil2, int precision, int tuning, int* out);
extern "C" int vfx_plan_resblock_geometry(int C, int T, int dil, int dil2, int precision, int* out) {
  return vfx_plan_resblock_geometry_tuned(C, T, dil, dil2, precision, 0, out);
}

extern "C" int vfx_plan_resblock_geometry_tuned(int C, int T, int dil, int dil2, int precision, int tuning, int* out) {
  try {
    VFX_CHECK(out && T > 0 && dil >= 1 && dil2 >= 0, "bad argument");
    ResBlockParams rp{};
    rp.B = 1;
    rp.T = T;
    rp.C = C;
    rp.dil = dil;
    rp.dil2 = dil2;
    rp.hionly = precision == 2;
    rp.tuning = tuning;
    if (precision == 2 && resblock_w64_supported(C)) rp.asrc = 1;
    // the trunk form the vocoder plan would give this layer (vocoder.cpp stack_trunk_f16)
    rp.x16 = (precision == 2 && !(tuning & VFX_TUNE_F32_TRUNK) && (C == 256 || C == 128 || (C == 64 && resblock_rw_tile(tuning) != 0))) ? 1 : 0;
    plan_resblock(rp);
    const int v[12] = {rp.fold, rp.TH, rp.W1, rp.TWo, rp.tiles_h, rp.tiles_w, rp.PW, rp.P, rp.tile_m, rp.rw, rp.patch_rows, rp.asrc};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_plan_conv_geometry(int Hg, int Wg, int ntaps, const int* dh, const int* dw, int* out) {
  try {
    VFX_CHECK(out && dh && dw && Hg > 0 && Wg > 0 && ntaps >= 1 && ntaps <= kMaxTaps, "bad argument");
    static float dummy;
    TapConvParams p{};
    p.B = 1;
    p.Hi = p.Hg = p.Ho = Hg;
    p.Wi = p.Wg = p.Wo = Wg;
    p.sh = p.sw = 1;
    p.Cout = 32;
    p.split = 1;
    p.out = &dummy;  // never dereferenced: host-side planning only
    p.nseg = 1;
    p.seg[0].C = 32;
    p.seg[0].ntaps = ntaps;
    for (int t = 0; t < ntaps; ++t) {
      p.seg[0].dh[t] = dh[t];
      p.seg[0].dw[t] = dw[t];
    }
    finish_params(p);
    const int v[6] = {p.TH, p.TW, p.PW, p.P, p.per_tap, p.tiles_h * p.tiles_w};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_plan_block2d_geometry(int C, int H, int W, int kind, int tuning, int* out) {
  try {
    VFX_CHECK(out && H > 0 && W > 0 && kind >= 0 && kind <= 2, "bad argument");
    ResBlockParams rp{};
    rp.B = 1;
    rp.H = H;
    rp.W = W;
    rp.C = C;
    rp.geo2d = 1;
    rp.in1 = kind == 1;
    rp.two_src = kind == 2;
    rp.tuning = tuning;
    plan_block2d(rp);
    const int v[8] = {rp.TH, rp.W1, rp.TWo, rp.tiles_h, rp.tiles_w, rp.PW, rp.P, rp.tile_m};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// Two consecutive ResStack layers (dilations dil, dil2) of the 16-bit mode at C = 64 as ONE launch (resblock_rw.hip, PAIR): the
// first layer's output never leaves the CU.  Weights / biases in PyTorch layout on the HOST: wa1, ba1, wa2, ba2 = first layer,
// wb1 .. bb2 = second layer.  Fails (returns 1) where the plan would not pair the layers.
extern "C" int vfx_op_resblock_pair(vfx_handle* h, const float* x, int B, int T, int C, const float* wa1, const float* ba1,
                                    const float* wa2, const float* ba2, int dil, const float* wb1, const float* bb1,
                                    const float* wb2, const float* bb2, int dil2, float slope, float* y, void* stream) {
  try {
    VFX_CHECK(h && x && y && wa1 && ba1 && wa2 && ba2 && wb1 && bb1 && wb2 && bb2 && B > 0 && T > 0, "bad argument");
    DeviceGuard device_guard_(h->device);
    VFX_CHECK(h->cfg.precision == 2 && (resblock_rw_pair_ok(C, dil, dil2, h->cfg.tuning) || resblock_r128_pair_ok(C, dil, dil2, h->cfg.tuning)),
              "vfx_op_resblock_pair: needs the 16-bit mode and a pair the plan would build (C = 64: dil <= 32, dil2 <= 62; C = 128: (1, 3))");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    std::vector<std::pair<int, int>> taps = {{0, 0}, {0, 1}, {0, 2}};
    ResBlockParams rp{};
    rp.x = x;
    rp.y = y;
    rp.w1 = sc.blob.upload(pack_conv(wa1, C, C, 1, 3, 0, C, taps, 2));
    rp.w2 = sc.blob.upload(pack_conv(wa2, C, C, 1, 3, 0, C, taps, 2));
    rp.b1 = sc.blob.upload(ba1, C);
    rp.b2 = sc.blob.upload(ba2, C);
    rp.w1b = sc.blob.upload(pack_conv(wb1, C, C, 1, 3, 0, C, taps, 2));
    rp.w2b = sc.blob.upload(pack_conv(wb2, C, C, 1, 3, 0, C, taps, 2));
    rp.b1b = sc.blob.upload(bb1, C);
    rp.b2b = sc.blob.upload(bb2, C);
    rp.slope = slope;
    rp.B = B;
    rp.T = T;
    rp.C = C;
    rp.hionly = 1;
    rp.flags = h->d_flags;
    rp.dil = dil;
    rp.dil2 = dil2;
    rp.tuning = h->cfg.tuning;
    const size_t nel = (size_t)B * T * C;
    if (handle_trunk_f16(h)) {
      rp.x = to_device_f16(sc.blob, x, nel, 1.f);
      run_raw_f16_trunk(rp, y, nel, slope, sc.blob, s);
    } else {
      float* dya = static_cast<float*>(sc.blob.alloc(nel * sizeof(_Float16)));
      rp.ya = dya;
      rp.act_slope = slope;
      plan_resblock(rp);
      ResBlockParams* d = static_cast<ResBlockParams*>(sc.blob.alloc(sizeof(ResBlockParams)));
      VFX_HIP(hipMemcpy(d, &rp, sizeof(rp), hipMemcpyHostToDevice));
      launch_resblock(rp, d, s);
      check_activated_output(y, dya, nel, slope, s);
    }
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// One fused 2-D ConvBlockRes (Cin == Cout = C in {32, 64}, identity shortcut; resblock.hip, G2 mode):
//   y = x + conv2(lrelu(bn2(conv1(lrelu(bn1(x))))));  x, y (B, H, W, C) on the device; w1, w2 in PyTorch layout (C, C, 3, 3)
//   and the folded BatchNorm affines sc*/sh* [C] on the HOST.
extern "C" int vfx_op_block2d(vfx_handle* h, const float* x, int B, int H, int W, int C, const float* w1, const float* sc1,
                              const float* sh1, const float* w2, const float* sc2, const float* sh2, float slope, float* y,
                              void* stream) {
  try {
  VFX_CHECK(h && x && y && w1 && w2 && sc1 && sh1 && sc2 && sh2 && B > 0 && H > 0 && W > 0, "bad argument");
  DeviceGuard device_guard_(h->device);
  VFX_CHECK(h->cfg.precision != 0 && block2d_supported(C), "vfx_op_block2d: needs a split-bf16 mode and C = 32 or 64");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Scratch sc;
  std::vector<std::pair<int, int>> taps;
  for (int kh = 0; kh < 3; ++kh)
    for (int kw = 0; kw < 3; ++kw) taps.push_back({kh, kw});
  ResBlockParams rp{};
  rp.x = x;
  rp.y = y;
  rp.w1 = sc.blob.upload(pack_conv(w1, C, C, 3, 3, 0, C, taps, 1));
  rp.w2 = sc.blob.upload(pack_conv(w2, C, C, 3, 3, 0, C, taps, 1));
  rp.sc1 = sc.blob.upload(sc1, C);
  rp.sh1 = sc.blob.upload(sh1, C);
  rp.sc2 = sc.blob.upload(sc2, C);
  rp.sh2 = sc.blob.upload(sh2, C);
  rp.slope = slope;
  rp.B = B;
  rp.H = H;
  rp.W = W;
  rp.C = C;
  rp.tuning = h->cfg.tuning;
  plan_block2d(rp);
  ResBlockParams* d = static_cast<ResBlockParams*>(sc.blob.alloc(sizeof(ResBlockParams)));
  VFX_HIP(hipMemcpy(d, &rp, sizeof(rp), hipMemcpyHostToDevice));
  launch_resblock(rp, d, s);
  if (const char* reps = getenv("VFX_OP_REPS")) {  // measurement aid: the same launch N more times between two events, average on stderr
    const int n = atoi(reps);
    hipEvent_t e0, e1;
    VFX_HIP(hipEventCreate(&e0));
    VFX_HIP(hipEventCreate(&e1));
    VFX_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < n; ++i) launch_resblock(rp, d, s);
    VFX_HIP(hipEventRecord(e1, s));
    VFX_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    VFX_HIP(hipEventElapsedTime(&ms, e0, e1));
    fprintf(stderr, "[vfx_op_block2d] %d launches: %.2f us each\n", n, 1000.0 * ms / (n > 0 ? n : 1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_conv_transpose(vfx_handle* h, const float* x, int B, int H, int W, int Cin, const float* weight,
                                     int Cout, int kh, int kw, int stride, int prune_w, const float* scale,
                                     const float* shift, int act, float slope, const float* bias, float* y,
                                     void* stream) {
  try {
    VFX_CHECK(h && x && weight && y, "NULL argument");
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const float* dbias = bias ? sc.blob.upload(bias, Cout) : nullptr;
    if (kh == 3 && kw == 3 && stride == 2 && !bias && H >= 2 && W >= 2 && Cout % 32 == 0 && !(h->cfg.tuning & VFX_TUNE_NO_FUSED_UNET)) {
      // the product's form (resunet.cpp, TrunkBuilder::upsample): all four parity classes as the PHASES of one launch, the output
      // addressed in units of Cout (out_cmul, phase_rows); VFX_TUNE_TWO_LAUNCH_UPSAMPLERS: the two column classes of a row class as
      // the phases of one launch -- even output width: the output viewed as (B, 2H, W, 2 Cout); odd width: out_cmul
      const int Ho = 2 * H, Wo = prune_w ? 2 * W : 2 * W + 1;
      const bool four = !(h->cfg.tuning & VFX_TUNE_TWO_LAUNCH_UPSAMPLERS);  // all four phases in one launch (either width)
      if (four) {
        TapConvParams p{};
        p.B = B;
        p.Hi = H;
        p.Wi = W;
        p.Ho = Ho;
        p.Wo = Wo;
        p.Cout = 4 * Cout;
        p.out_cmul = Cout;
        p.phase_rows = 1;
        p.sh = 2;
        p.sw = 2;
        p.Hg = (Ho + 1) / 2;
        p.Wg = (Wo + 1) / 2;
        p.out = y;
        p.nseg = 1;
        std::vector<TapSeg> phases(4);
        for (int ph = 0; ph < 4; ++ph) {
          TapSeg& S = phases[ph];
          S = TapSeg{};
          std::vector<std::pair<int, int>> taps;
          for (int r = ph >> 1; r < 3; r += 2)
            for (int c = ph & 1; c < 3; c += 2) {
              S.dh[taps.size()] = -(r / 2);
              S.dw[taps.size()] = -(c / 2);
              taps.push_back({r, c});
            }
          S.ntaps = (int)taps.size();
          fill_seg(S, x, Cin, scale, shift, act, slope, sc.blob);
          S.wt = sc.blob.upload(pack_conv_transposed(weight, Cin, Cout, 3, 3, taps, h->cfg.precision == 2 ? 2 : (h->cfg.precision != 0)));
        }
        p.seg[0] = phases[0];
        run_phased(h, p, phases, sc.blob, s);
      }
      for (int a = 0; a < 2 && !four; ++a) {
        TapConvParams p{};
        p.B = B;
        p.Hi = H;
        p.Wi = W;
        p.Ho = Ho;
        p.Cout = 2 * Cout;
        p.sh = 2;
        p.oh0 = a;
        p.ow0 = 0;
        p.Hg = (Ho - a + 1) / 2;
        if (prune_w) {
          p.Wo = W;
          p.sw = 1;
          p.Wg = W;
        } else {
          p.Wo = Wo;
          p.sw = 2;
          p.Wg = W + 1;
          p.out_cmul = Cout;
        }
        p.out = y;
        p.nseg = 1;
        std::vector<TapSeg> phases(2);
        for (int b = 0; b < 2; ++b) {
          TapSeg& S = phases[b];
          S = TapSeg{};
          std::vector<std::pair<int, int>> taps;
          for (int r = a; r < 3; r += 2)
            for (int c = b; c < 3; c += 2) {
              S.dh[taps.size()] = -(r / 2);
              S.dw[taps.size()] = -(c / 2);
              taps.push_back({r, c});
            }
          S.ntaps = (int)taps.size();
          fill_seg(S, x, Cin, scale, shift, act, slope, sc.blob);
          S.wt = sc.blob.upload(pack_conv_transposed(weight, Cin, Cout, 3, 3, taps, h->cfg.precision == 2 ? 2 : (h->cfg.precision != 0)));
        }
        p.seg[0] = phases[0];
        run_phased(h, p, phases, sc.blob, s);
      }
    } else if (kh == 3 && kw == 3 && stride == 2) {
      const int Ho = 2 * H, Wo = prune_w ? 2 * W : 2 * W + 1;
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
          TapConvParams p{};
          TapSeg& S = p.seg[0];
          std::vector<std::pair<int, int>> taps;
          for (int r = a; r < 3; r += 2)
            for (int c = b; c < 3; c += 2) {
              S.dh[taps.size()] = -(r / 2);
              S.dw[taps.size()] = -(c / 2);
              taps.push_back({r, c});
            }
          S.ntaps = (int)taps.size();
          fill_seg(S, x, Cin, scale, shift, act, slope, sc.blob);
          S.wt = sc.blob.upload(pack_conv_transposed(weight, Cin, Cout, 3, 3, taps, h->cfg.precision == 2 ? 2 : (h->cfg.precision != 0)));
          p.nseg = 1;
          p.B = B;
          p.Hi = H;
          p.Wi = W;
          p.Ho = Ho;
          p.Wo = Wo;
          p.Cout = Cout;
          p.sh = p.sw = 2;
          p.oh0 = a;
          p.ow0 = b;
          p.Hg = (Ho - a + 1) / 2;
          p.Wg = (Wo - b + 1) / 2;
          p.bias = dbias;
          p.out = y;
          run_one(h, p, sc.blob, s);
        }
    } else {
      VFX_CHECK(kh == 1 && H == 1 && kw == 2 * stride, "vfx_op_conv_transpose: unsupported geometry");
      const int sN = stride, pad = sN / 2 + sN % 2;
      for (int r = 0; r < sN; ++r) {
        TapConvParams p{};
        TapSeg& S = p.seg[0];
        std::vector<std::pair<int, int>> taps;
        for (int e = -2; e <= 2; ++e) {
          const int k = sN * e + r + pad;
          if (k >= 0 && k < 2 * sN) {
            S.dh[taps.size()] = 0;
            S.dw[taps.size()] = -e;
            taps.push_back({0, k});
          }
        }
        S.ntaps = (int)taps.size();
        fill_seg(S, x, Cin, scale, shift, act, slope, sc.blob);
        S.wt = sc.blob.upload(pack_conv_transposed(weight, Cin, Cout, 1, kw, taps, h->cfg.precision == 2 ? 2 : (h->cfg.precision != 0)));
        p.nseg = 1;
        p.B = B;
        p.Hi = p.Hg = p.Ho = 1;
        p.Wi = p.Wg = W;
        p.Wo = W * sN;
        p.Cout = Cout;
        p.sh = 1;
        p.sw = sN;
        p.ow0 = r;
        p.bias = dbias;
        p.out = y;
        run_one(h, p, sc.blob, s);
      }
    }
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// ---- the vocoder's launches as the plan builds them (vocoder.cpp: voc_upsample_params, voc_conv1d_params, voc_resblock_params, launch_voc_final)
namespace {
uint16_t bf16_rne_host(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf16_to_f32_host(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
float act_host(float v, int act, float slope) {
  if (act == ACT_ELU) return v > 0.f ? v : expm1f(v);
  if (act == ACT_LEAKY) return v > 0.f ? v : v * slope;
  return v;
}

// Device fp32 tensor (npix, C) -> its ACTIVATED form act(x) in the handle's operand form (TapConvParams::out_act): 16-bit mode an fp16
// tensor, split-bf16 per pixel and 32-channel chunk [32 hi bf16 | 32 lo bf16] (lo = bf16(v - hi)), fp32 the activated floats.
float* to_device_act(const vfx_handle* h, DeviceBlob& blob, const float* dx, size_t npix, int C, int act, float slope) {
  const size_t n = npix * C;
  std::vector<float> hx(n);
  VFX_HIP(hipMemcpy(hx.data(), dx, n * sizeof(float), hipMemcpyDeviceToHost));
  for (float& v : hx) v = act_host(v, act, slope);
  if (h->cfg.precision == 2) {
    std::vector<_Float16> hh(n);
    for (size_t i = 0; i < n; ++i) hh[i] = (_Float16)std::min(std::max(hx[i], -65504.f), 65504.f);
    void* d = blob.alloc(n * sizeof(_Float16));
    VFX_HIP(hipMemcpy(d, hh.data(), n * sizeof(_Float16), hipMemcpyHostToDevice));
    return static_cast<float*>(d);
  }
  if (h->cfg.precision == 1) {
    std::vector<uint16_t> q(2 * n);
    for (size_t i = 0; i < n; ++i) {
      const size_t base = i / 32 * 64, c = i % 32;  // (C % 32 == 0: a chunk never straddles two pixels)
      const uint16_t hi = bf16_rne_host(hx[i]);
      q[base + c] = hi;
      q[base + 32 + c] = bf16_rne_host(hx[i] - bf16_to_f32_host(hi));
    }
    void* d = blob.alloc(q.size() * sizeof(uint16_t));
    VFX_HIP(hipMemcpy(d, q.data(), q.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return static_cast<float*>(d);
  }
  return blob.upload(hx.data(), n);
}
// bytes of an activated tensor of n elements in the handle's operand form
size_t act_bytes(const vfx_handle* h, size_t n) { return h->cfg.precision == 2 ? n * 2 : n * 4; }
// ... and back: the caller's fp32 tensor receives the stored values (form 2: fp16 widened, 1: hi + lo, 0: fp32), NaN patterns included
void act_to_f32(int form, const float* dact, size_t n, float* dy) {
  std::vector<float> hy(n);
  if (form == 2) {
    std::vector<_Float16> hh(n);
    VFX_HIP(hipMemcpy(hh.data(), dact, n * sizeof(_Float16), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) hy[i] = (float)hh[i];
  } else if (form == 1) {
    std::vector<uint16_t> q(2 * n);
    VFX_HIP(hipMemcpy(q.data(), dact, q.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      const size_t base = i / 32 * 64, c = i % 32;
      hy[i] = bf16_to_f32_host(q[base + c]) + bf16_to_f32_host(q[base + 32 + c]);
    }
  } else {
    VFX_HIP(hipMemcpy(hy.data(), dact, n * sizeof(float), hipMemcpyDeviceToHost));
  }
  VFX_HIP(hipMemcpy(dy, hy.data(), n * sizeof(float), hipMemcpyHostToDevice));
}
const int* upload_lens(DeviceBlob& blob, const int* lens, int B) {
  return lens ? blob.upload_i(std::vector<int>(lens, lens + B)) : nullptr;
}
// a tap convolution set up the way PlanBuilder::add_conv does it for the vocoder (no split-K: PlanBuilder::no_splitk)
void run_voc_conv(vfx_handle* h, TapConvParams& p, DeviceBlob& blob, hipStream_t s) {
  p.split = h->cfg.precision != 0;
  p.flags = h->d_flags;
  p.tuning = h->cfg.tuning;
  finish_params(p);
  std::vector<ConvStage> st(p.nstages);
  build_stages(p, h->d_ones, h->d_zeros, st.data());
  ConvStage* ds = static_cast<ConvStage*>(blob.alloc(st.size() * sizeof(ConvStage)));
  VFX_HIP(hipMemcpy(ds, st.data(), st.size() * sizeof(ConvStage), hipMemcpyHostToDevice));
  p.stages = ds;
  p.ksplit = 0;
  TapConvParams* d = static_cast<TapConvParams*>(blob.alloc(sizeof(TapConvParams)));
  VFX_HIP(hipMemcpy(d, &p, sizeof(p), hipMemcpyHostToDevice));
  launch_conv(p, d, s);
}
}  // namespace

extern "C" int vfx_op_voc_upsample(vfx_handle* h, const float* x, int B, int T, int Cin, const float* weight, const float* bias, int stride,
                                   float up_slope, int src_act, int want_raw, int want_act, float act_slope, const int* lens, float* y,
                                   float* ya, int* used_up16, void* stream) {
  try {
    VFX_CHECK(h && x && weight && bias && B > 0 && T > 0 && stride >= 1 && Cin % 64 == 0 && (want_raw || want_act) && (!want_raw || y) &&
                  (!want_act || ya),
              "vfx_op_voc_upsample: bad argument");
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    vfx_config cfg = h->cfg;
    cfg.voc_up_slope = up_slope;
    const int Cout = Cin / 2;
    const size_t nout = (size_t)B * T * stride * Cout;
    const VocConvW up = pack_voc_upsampler(cfg, sc.blob, weight, bias, Cin, stride, src_act != 0);
    const float* src = src_act ? to_device_act(h, sc.blob, x, (size_t)B * T, Cin, ACT_LEAKY, up_slope) : x;
    float* dact = nullptr;
    if (want_act) {  // NaN patterns (0xff bytes in every form): what the launch leaves unwritten stays NaN
      dact = static_cast<float*>(sc.blob.alloc(act_bytes(h, nout)));
      VFX_HIP(hipMemset(dact, 0xff, act_bytes(h, nout)));
    }
    std::vector<TapSeg> phases;
    TapConvParams p = voc_upsample_params(cfg, up, stride, B, T, src, src_act != 0, want_raw ? y : nullptr, dact, act_slope,
                                          upload_lens(sc.blob, lens, B), 1, phases);
    // the rest of PlanBuilder::add_conv_phased + bind_plan, with the plan's kernel choice
    p.split = h->cfg.precision != 0;
    p.flags = h->d_flags;
    p.tuning = h->cfg.tuning;
    p.nphase = stride;
    p.cout_phase = Cout;
    finish_params(p);
    VFX_CHECK(!p.per_tap, "phased conv: the union of the phases' taps does not fit one patch");
    p.ksplit = 0;
    p.up16 = upsample16_selected(p, phases) ? 1 : 0;
    std::vector<ConvStage> st((size_t)p.nstages * p.nphase);
    for (int r = 0; r < p.nphase; ++r) {
      TapConvParams q = p;
      q.seg[0] = phases[r];
      build_stages(q, h->d_ones, h->d_zeros, st.data() + (size_t)r * p.nstages);
    }
    ConvStage* ds = static_cast<ConvStage*>(sc.blob.alloc(st.size() * sizeof(ConvStage)));
    VFX_HIP(hipMemcpy(ds, st.data(), st.size() * sizeof(ConvStage), hipMemcpyHostToDevice));
    p.stages = ds;
    TapConvParams* d = static_cast<TapConvParams*>(sc.blob.alloc(sizeof(TapConvParams)));
    VFX_HIP(hipMemcpy(d, &p, sizeof(p), hipMemcpyHostToDevice));
    launch_conv(p, d, s);
    VFX_HIP(hipStreamSynchronize(s));
    if (dact) act_to_f32(h->cfg.precision, dact, nout, ya);
    if (used_up16) *used_up16 = p.up16;
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_voc_conv1d(vfx_handle* h, const float* x, int B, int T, int Cin, const float* weight, const float* bias, int Cout,
                                 int K, int dil, int reflect, int src_act, int act, float slope, const float* residual, int residual_act,
                                 int want_raw, int next_act, float next_slope, const int* lens, float* y, float* ya, void* stream) {
  try {
    VFX_CHECK(h && x && weight && bias && B > 0 && T > 0 && (K == 3 || K == 7) && dil >= 1 && (want_raw || next_act != ACT_NONE) &&
                  (!want_raw || y) && (next_act == ACT_NONE || ya) && (!residual_act || residual),
              "vfx_op_voc_conv1d: bad argument");
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const vfx_config& cfg = h->cfg;
    const size_t nout = (size_t)B * T * Cout;
    const VocConvW cw = pack_voc_conv1d(cfg, sc.blob, weight, bias, Cin, Cout, K, src_act != 0);
    const float* src = src_act ? to_device_act(h, sc.blob, x, (size_t)B * T, Cin, act, slope) : x;
    // residual_act: the activated fp16 trunk fp16(LeakyReLU(residual, res_slope)) of the 16-bit mode
    const float* res = residual && residual_act ? to_device_f16(sc.blob, residual, nout, cfg.voc_res_slope) : residual;
    float* dact = nullptr;
    if (next_act != ACT_NONE) {
      dact = static_cast<float*>(sc.blob.alloc(act_bytes(h, nout)));
      VFX_HIP(hipMemset(dact, 0xff, act_bytes(h, nout)));
    }
    TapConvParams p = voc_conv1d_params(cfg, cw, B, T, K, dil, reflect != 0, src, src_act != 0, act, slope, res, residual_act != 0,
                                        want_raw ? y : nullptr, dact, next_act, next_slope, upload_lens(sc.blob, lens, B), 1);
    run_voc_conv(h, p, sc.blob, s);
    VFX_HIP(hipStreamSynchronize(s));
    if (dact) act_to_f32(h->cfg.precision, dact, nout, ya);
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_voc_final(vfx_handle* h, const float* x, int B, int T, int C, const float* weight, float bias, float slope, int x_f16,
                                const int* lens, float* wav, float* peak, void* stream) {
  try {
    VFX_CHECK(h && x && weight && wav && B > 0 && T > 0, "vfx_op_voc_final: bad argument");
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    std::vector<float> wt(7 * (size_t)C);  // (1, C, 7) -> [7][C], as build_vocoder_weights packs the final conv
    for (int k = 0; k < 7; ++k)
      for (int ch = 0; ch < C; ++ch) wt[k * C + ch] = weight[ch * 7 + k];
    const float* src = x_f16 ? to_device_f16(sc.blob, x, (size_t)B * T * C, 1.f) : x;
    launch_voc_final(src, x_f16 ? 1 : 0, B, T, C, sc.blob.upload(wt), bias, slope, wav,
                     reinterpret_cast<unsigned*>(peak), s, upload_lens(sc.blob, lens, B), 1);
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_plan_voc_upsampler_kernel(int Cin, int Cout, int s, int T, int precision, int tuning) {
  try {
    VFX_CHECK(Cin > 0 && Cin % 64 == 0 && Cout == Cin / 2 && s >= 1 && T > 0 && precision >= 0 && precision <= 2, "bad argument");
    vfx_config cfg{};
    VFX_CHECK(vfx_default_config(&cfg) == 0, "no default config");
    cfg.precision = precision;
    cfg.tuning = tuning;
    return voc_plan_upsampler_kernel(cfg, Cin, s, T);
  } catch (const vfx::Error&) {
    return -1;
  }
}

// One fused ResStack launch (a layer, or a pair: dil2 > 0) the way build_vocoder adds it: voc_resblock_params + plan_resblock +
// launch_resblock, the trunk in the form the handle gives this width.  Both outputs live in ONE device buffer between guard zones,
// all of it NaN patterns before the launch: [guard | y | guard | ya | guard]; a guard byte -- or a byte of an output the launch was
// not given -- that changed is an error of the call.
extern "C" int vfx_op_voc_resblock(vfx_handle* h, const float* x, int B, int T, int C, const float* w1, const float* b1, const float* w2,
                                   const float* b2, int dil, const float* w1b, const float* b1b, const float* w2b, const float* b2b,
                                   int dil2, float slope, float act_slope, int want_raw, int want_act, const int* lens, int lens_mul,
                                   float* y, float* ya, int* info, void* stream) {
  try {
    VFX_CHECK(h && x && w1 && b1 && w2 && b2 && B > 0 && T > 0 && C > 0 && dil >= 1 && dil2 >= 0 && (want_raw || want_act) &&
                  (!want_raw || y) && (!want_act || ya) && lens_mul >= 1 && (dil2 == 0 || (w1b && b1b && w2b && b2b)),
              "vfx_op_voc_resblock: bad argument");
    for (int b = 0; lens && b < B; ++b)
      VFX_CHECK(lens[b] >= 0 && (int64_t)lens[b] * lens_mul <= T, "vfx_op_voc_resblock: clip %d has %d x %d positions (need 0 .. T = %d)", b,
                lens[b], lens_mul, T);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    vfx_config cfg = h->cfg;
    cfg.voc_res_slope = slope;
    const int kind = voc_resblock_kind(cfg, C);
    VFX_CHECK(kind != VOC_RES_TWO_LAUNCHES, "vfx_op_voc_resblock: the plan of this handle runs a %d-channel layer as two k_conv launches", C);
    const bool wide = kind == VOC_RES_FUSED_WIDE;
    // want_act: a stack in front of an upsampler; otherwise the last stage's form (the tail reads the raw trunk)
    const bool last_stage = !want_act;
    const bool t16 = voc_resblock_trunk_f16(cfg, C, last_stage);
    const size_t nel = (size_t)B * T * C;
    const VocResLayer l1{pack_voc_conv1d(cfg, sc.blob, w1, b1, C, C, 3, wide), pack_voc_conv1d(cfg, sc.blob, w2, b2, C, C, 3, wide)};
    VocResLayer l2;
    if (dil2 > 0) l2 = {pack_voc_conv1d(cfg, sc.blob, w1b, b1b, C, C, 3, wide), pack_voc_conv1d(cfg, sc.blob, w2b, b2b, C, C, 3, wide)};
    const float* dx = wide ? (t16 ? nullptr : x) : (t16 ? to_device_f16(sc.blob, x, nel, 1.f) : x);
    const float* dxa = wide ? to_device_f16(sc.blob, x, nel, slope) : nullptr;
    const bool y_f16 = t16 && !wide;
    const size_t guard = 1 << 16, ybytes = (nel * (y_f16 ? 2 : 4) + 255) / 256 * 256, abytes = (nel * 2 + 255) / 256 * 256;
    const size_t yoff = guard, aoff = yoff + ybytes + guard, total = aoff + abytes + guard;
    char* buf = static_cast<char*>(sc.blob.alloc(total));
    VFX_HIP(hipMemset(buf, 0xff, total));
    float* dy = want_raw ? reinterpret_cast<float*>(buf + yoff) : nullptr;
    float* dya = want_act ? reinterpret_cast<float*>(buf + aoff) : nullptr;
    ResBlockParams rp = voc_resblock_params(cfg, C, last_stage, l1, dil2 > 0 ? &l2 : nullptr, B, T, dil, dil2, dx, dxa, dy, dya, act_slope,
                                            upload_lens(sc.blob, lens, B), lens_mul);
    rp.flags = h->d_flags;
    plan_resblock(rp);
    if (info) {
      const int v[12] = {rp.rw, rp.r128, rp.asrc, rp.fold, rp.tile_m, rp.TWo, rp.TH, rp.tiles_h, rp.tiles_w, rp.x16, rp.W1, rp.patch_rows};
      for (int i = 0; i < 12; ++i) info[i] = v[i];
    }
    ResBlockParams* d = static_cast<ResBlockParams*>(sc.blob.alloc(sizeof(ResBlockParams)));
    VFX_HIP(hipMemcpy(d, &rp, sizeof(rp), hipMemcpyHostToDevice));
    launch_resblock(rp, d, s);
    VFX_HIP(hipStreamSynchronize(s));
    std::vector<unsigned char> hb(total);
    VFX_HIP(hipMemcpy(hb.data(), buf, total, hipMemcpyDeviceToHost));
    auto untouched = [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i)
        if (hb[i] != 0xff) return false;
      return true;
    };
    VFX_CHECK(untouched(0, yoff) && untouched(yoff + (want_raw ? nel * (y_f16 ? 2 : 4) : 0), aoff) &&
                  untouched(aoff + (want_act ? nel * 2 : 0), total),
              "vfx_op_voc_resblock: the launch wrote outside its outputs");
    std::vector<float> hy(nel);
    auto widen = [&](size_t off, bool f16, float* dst) {
      if (f16) {
        const _Float16* p16 = reinterpret_cast<const _Float16*>(hb.data() + off);
        for (size_t i = 0; i < nel; ++i) hy[i] = (float)p16[i];
      } else {
        memcpy(hy.data(), hb.data() + off, nel * sizeof(float));
      }
      VFX_HIP(hipMemcpy(dst, hy.data(), nel * sizeof(float), hipMemcpyHostToDevice));
    };
    if (want_raw) widen(yoff, y_f16, y);
    if (want_act) widen(aoff, true, ya);
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// ---- the ResUNet plans' launches, one piece at a time, built by the plan's own builder (resunet.cpp: build_unet_piece) -----------------
extern "C" int vfx_op_unet_piece(vfx_handle* h, int model, const char* piece, int B, int H, int W, int arg, int short_clip, const int* lens,
                                 const float* const* in, const int64_t* in_n, int nin, float* const* out, const int64_t* out_n, int nout,
                                 float* h_out, int64_t h_n, int* h_form, int* launches, int cap, int* nlaunch, void* stream) {
  try {
    VFX_CHECK(h && piece && in && in_n && out && out_n && (model == VFX_MODEL_UNET_MEL || model == VFX_MODEL_UNET_SPEC),
              "vfx_op_unet_piece: bad argument");
    VFX_CHECK(h->unet[model], "vfx_op_unet_piece: the ResUNet weights of model %d are not finalized", model);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    Plan plan;
    PlanBuilder pb{h, &plan, {}};
    pb.short_clip = short_clip;
    pb.lens_t = upload_lens(sc.blob, lens, B);
    UNetPiece pc{};
    pc.name = piece;
    pc.B = B;
    pc.H = H;
    pc.W = W;
    pc.arg = arg;
    build_unet_piece(pb, *h->unet[model], pc);
    // the caller's tensors must be the plan's buffers element for element: nothing below copies by any other count
    VFX_CHECK(nin == pc.nin && nout == pc.nout, "vfx_op_unet_piece: '%s' has %d inputs and %d outputs", piece, pc.nin, pc.nout);
    for (int i = 0; i < nin; ++i)
      VFX_CHECK(in[i] && in_n[i] == pc.in_n[i], "vfx_op_unet_piece: input %d of '%s' has %lld floats", i, piece, (long long)pc.in_n[i]);
    for (int i = 0; i < nout; ++i)
      VFX_CHECK(out[i] && out_n[i] == pc.out_n[i], "vfx_op_unet_piece: output %d of '%s' has %lld floats", i, piece, (long long)pc.out_n[i]);
    VFX_CHECK(pc.h_n == 0 || !h_out || h_n == pc.h_n, "vfx_op_unet_piece: the intermediate tensor of '%s' has %lld floats", piece,
              (long long)pc.h_n);
    plan.arena_bytes = pb.arena.high;
    bind_plan(h, plan);
    char* base = plan.bound_base;
    // NaN patterns everywhere first (what no launch writes stays NaN, split-K workspace included), then the inputs
    VFX_HIP(hipMemsetAsync(base, 0xff, plan.arena_bytes, s));
    for (int i = 0; i < nin; ++i)
      VFX_HIP(hipMemcpyAsync(base + pc.in_off[i], in[i], (size_t)pc.in_n[i] * sizeof(float), hipMemcpyDeviceToDevice, s));
    RunCtx ctx{s, {}, h->d_flags, nullptr};
    plan.run(ctx);
    for (int i = 0; i < nout; ++i)
      VFX_HIP(hipMemcpyAsync(out[i], base + pc.out_off[i], (size_t)pc.out_n[i] * sizeof(float), hipMemcpyDeviceToDevice, s));
    VFX_HIP(hipStreamSynchronize(s));
    if (pc.h_n && h_out)
      act_to_f32(pc.h_form == 1 && h->cfg.precision != 0 ? 1 : 0, reinterpret_cast<const float*>(base + pc.h_off), (size_t)pc.h_n, h_out);
    if (h_form) *h_form = pc.h_n ? pc.h_form : -1;
    const int n = describe_unet_launches(plan, launches, launches ? cap : 0);
    if (nlaunch) *nlaunch = n;
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// ---- the bi_gru / dnn plans' launches, one at a time, built by the plan's own builder (analysis.hip: build_analysis_piece) -------------
extern "C" int vfx_op_analysis_piece(vfx_handle* h, int model, const char* piece, int B, int T, const int* lens, const float* const* in,
                                     const int64_t* in_n, int nin, float* out, int64_t out_n, void* stream) {
  try {
    VFX_CHECK(h && piece && in && in_n && out && B > 0 && T > 0 && (model == VFX_MODEL_GRU_MEL || model == VFX_MODEL_DNN_MEL),
              "vfx_op_analysis_piece: bad argument");
    VFX_CHECK(h->analysis[model - VFX_MODEL_GRU_MEL], "vfx_op_analysis_piece: the weights of model %d are not finalized", model);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Plan plan;
    PlanBuilder pb{h, &plan, {}};
    if (lens) {  // as vfx_analysis_mel_1: the handle's own row of frame counts, filled in stream order
      VFX_CHECK(B <= kMaxVarlenClips, "vfx_op_analysis_piece: %d clips with frame counts (at most %d)", B, kMaxVarlenClips);
      for (int b = 0; b < B; ++b)
        VFX_CHECK(lens[b] >= 1 && lens[b] <= T, "vfx_op_analysis_piece: clip %d has %d frames (need 1 <= frames <= T = %d)", b, lens[b], T);
      int* const d_f = h->lens_row(LENS_ANALYSIS_FRAMES);
      launch_set_frames(d_f, lens, B, s);
      pb.lens_t = d_f;
    }
    AnalysisPiece pc{};
    pc.name = piece;
    pc.B = B;
    pc.T = T;
    build_analysis_piece(pb, model, pc);
    // the caller's tensors must be the plan's buffers element for element: nothing below copies by any other count
    VFX_CHECK(nin == pc.nin, "vfx_op_analysis_piece: '%s' has %d inputs", piece, pc.nin);
    for (int i = 0; i < nin; ++i)
      VFX_CHECK(in[i] && in_n[i] == pc.in_n[i], "vfx_op_analysis_piece: input %d of '%s' has %lld floats", i, piece, (long long)pc.in_n[i]);
    VFX_CHECK(out_n == pc.out_n, "vfx_op_analysis_piece: the output of '%s' has %lld floats", piece, (long long)pc.out_n);
    plan.arena_bytes = pb.arena.high;
    bind_plan(h, plan);
    char* base = plan.bound_base;
    // NaN patterns everywhere first (what the launch does not write stays NaN), then the inputs
    VFX_HIP(hipMemsetAsync(base, 0xff, plan.arena_bytes, s));
    for (int i = 0; i < nin; ++i)
      VFX_HIP(hipMemcpyAsync(base + pc.in_off[i], in[i], (size_t)pc.in_n[i] * sizeof(float), hipMemcpyDeviceToDevice, s));
    RunCtx ctx{s, {}, h->d_flags, nullptr};
    plan.run(ctx);
    VFX_HIP(hipMemcpyAsync(out, base + pc.out_off, (size_t)pc.out_n * sizeof(float), hipMemcpyDeviceToDevice, s));
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_plan_unet_piece(const char* piece, int B, int H, int W, int arg, int short_clip, int precision, int tuning, int* launches,
                                   int cap, int* nlaunch) {
  try {
    VFX_CHECK(piece && nlaunch && precision >= 0 && precision <= 2, "vfx_plan_unet_piece: bad argument");
    vfx_handle hh;  // never touches a device: build_unet_piece only plans
    VFX_CHECK(vfx_default_config(&hh.cfg) == 0, "no default config");
    hh.cfg.precision = precision;
    hh.cfg.tuning = tuning;
    UNetWeights shapes = unet_weight_shapes();
    static float dummy;  // never dereferenced (host-side planning only): a block with a shortcut has a bias
    auto mark = [](ConvBlockW& w) { if (w.shortcut) w.bsc = &dummy; };
    for (auto& lv : shapes.enc) for (auto& w : lv) mark(w);
    for (auto& D : shapes.dec) for (auto& w : D.blocks) mark(w);
    shapes.c1_bsc = &dummy;
    Plan plan;
    PlanBuilder pb{&hh, &plan, {}};
    pb.short_clip = short_clip;
    UNetPiece pc{};
    pc.name = piece;
    pc.B = B;
    pc.H = H;
    pc.W = W;
    pc.arg = arg;
    build_unet_piece(pb, shapes, pc);
    *nlaunch = describe_unet_launches(plan, launches, launches ? cap : 0);
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// ---- the STFT / ISTFT front end and the glue launches of a restore call, one launcher each with the handle's tables -------------------
extern "C" int vfx_op_stft(vfx_handle* h, const float* wav, int B, int L, int T, const int* lens, float eps, int log10_mel, float* mel,
                           float* sp, float* cosp, float* sinp, void* stream) {
  try {
    VFX_CHECK(h && wav && B > 0 && T > 0 && (mel || sp || cosp || sinp) && eps >= 0.f, "vfx_op_stft: bad argument");
    const int hop = h->cfg.hop, half = h->cfg.n_fft / 2;
    VFX_CHECK(L > half, "vfx_op_stft: clips too short for reflect padding (L = %d)", L);
    VFX_CHECK(lens || T == L / hop + 1, "vfx_op_stft: without lens, T is L / hop + 1 = %d", L / hop + 1);
    for (int b = 0; lens && b < B; ++b)
      VFX_CHECK(lens[b] > half && lens[b] <= L, "vfx_op_stft: clip %d has %d samples (need %d .. L = %d)", b, lens[b], half + 1, L);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    launch_stft_mel(h->fe, wav, B, L, T, mel, sp, cosp, sinp, log10_mel, hop, eps, s, upload_lens(sc.blob, lens, B));
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_istft(vfx_handle* h, const float* re, const float* im, int B, int T, int L, const int* lens, float* wav,
                            void* stream) {
  try {
    VFX_CHECK(h && re && im && wav && B > 0 && T > 0 && L > 0, "vfx_op_istft: bad argument");
    for (int b = 0; lens && b < B; ++b)
      VFX_CHECK(lens[b] >= 1 && lens[b] <= L, "vfx_op_istft: clip %d has %d samples (need 1 .. L = %d)", b, lens[b], L);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    launch_istft(h->fe, re, im, B, T, L, h->cfg.hop, wav, s, upload_lens(sc.blob, lens, B));
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_debug_resample_each_layout(vfx_handle* h, int natural) {
  if (!h) return 1;
  h->rs_natural_taps = natural != 0;
  return 0;
}

extern "C" int vfx_plan_stft_frames_per_group(int64_t frames) { return frames > 0 ? frames_per_group(frames) : -1; }

extern "C" int vfx_plan_istft_grid(int B, int T, int L, int* out) {
  try {
    VFX_CHECK(B > 0 && T > 0 && L > 0 && out, "vfx_plan_istft_grid: bad argument");
    vfx_config cfg{};
    VFX_CHECK(vfx_default_config(&cfg) == 0, "no default config");
    const IstftGrid g = istft_grid(B, T, L, cfg.hop);
    out[0] = g.IH;
    out[1] = g.groups;
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_from_log(vfx_handle* h, const float* logmel, const float* mel_in, int B, int T, int unify, const int* lens_t,
                               float* mel_out, void* stream) {
  try {
    VFX_CHECK(h && logmel && mel_out && B > 0 && T > 0 && (!unify || mel_in), "vfx_op_from_log: bad argument");
    for (int b = 0; lens_t && b < B; ++b)
      VFX_CHECK(lens_t[b] >= 1 && lens_t[b] <= T, "vfx_op_from_log: clip %d has %d frames (need 1 .. T = %d)", b, lens_t[b], T);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    float* sums = static_cast<float*>(sc.blob.alloc(2 * (size_t)B * sizeof(float)));
    launch_from_log(logmel, mel_in, B, T, unify ? 1 : 0, sums, mel_out, s, upload_lens(sc.blob, lens_t, B));
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_voc_prep(vfx_handle* h, const float* mel, int B, int T, int Tp, const int* lens_t, float* cond, void* stream) {
  try {
    VFX_CHECK(h && mel && cond && B > 0 && T > 0 && Tp >= T, "vfx_op_voc_prep: bad argument");
    VFX_CHECK(h->cfg.n_mels == 128 && h->fe.voc_inv_weight, "vfx_op_voc_prep: the handle has no band weights");
    for (int b = 0; lens_t && b < B; ++b)
      VFX_CHECK(lens_t[b] >= 0 && lens_t[b] <= T, "vfx_op_voc_prep: clip %d has %d frames (need 0 .. T = %d)", b, lens_t[b], T);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    launch_voc_prep(mel, B, T, Tp, h->fe.voc_inv_weight, h->cfg.voc_amp_floor, h->cfg.voc_min_db, h->cfg.voc_norm_range, cond, s,
                    upload_lens(sc.blob, lens_t, B));
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_peak_trim(vfx_handle* h, const float* wav_long, int B, int64_t Llong, int L, const float* peak, const int* lens_l,
                                const int* lens_tp, float* out, void* stream) {
  try {
    VFX_CHECK(h && wav_long && peak && out && B > 0 && L > 0 && Llong >= L && (!lens_l == !lens_tp), "vfx_op_peak_trim: bad argument");
    const int hop = h->cfg.hop;
    for (int b = 0; lens_l && b < B; ++b)  // the clip's vocoder output lies inside its row, and its centre crop inside that
      VFX_CHECK(lens_l[b] >= 0 && lens_l[b] <= L && (int64_t)lens_tp[b] * hop <= Llong && (int64_t)lens_tp[b] * hop >= lens_l[b],
                "vfx_op_peak_trim: clip %d: %d samples from %d vocoder frames do not fit (L = %d, Llong = %lld)", b, lens_l[b], lens_tp[b],
                L, (long long)Llong);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const float* d_peak = sc.blob.upload(peak, B);
    if (lens_l)
      launch_peak_trim_varlen(wav_long, B, Llong, L, hop, upload_lens(sc.blob, lens_l, B), upload_lens(sc.blob, lens_tp, B), d_peak, out,
                              s, h->d_flags);
    else
      launch_peak_trim(wav_long, B, Llong, L, d_peak, out, s, h->d_flags);
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// one column of k_score_final's (B, 9) output -> out (B)
static void score_column(const ScoreFinalArgs& a0, int B, int col, DeviceBlob& blob, double* out, hipStream_t s) {
  ScoreFinalArgs a = a0;
  a.out = static_cast<double*>(blob.alloc((size_t)B * VFX_N_AUDIO_METRICS * sizeof(double)));
  launch_score_final(a, B, s);
  VFX_HIP(hipMemcpy2DAsync(out, sizeof(double), a.out + col, VFX_N_AUDIO_METRICS * sizeof(double), sizeof(double), B,
                           hipMemcpyDeviceToDevice, s));
  VFX_HIP(hipStreamSynchronize(s));
}

extern "C" int vfx_op_ssim(vfx_handle* h, const float* est, const float* target, int B, int T, int F, const int* rows, double* out,
                           void* stream) {
  try {
    VFX_CHECK(h && est && target && rows && out && B > 0 && B <= 65535 && T >= 7 && F >= 7, "vfx_op_ssim: bad argument");
    for (int b = 0; b < B; ++b) VFX_CHECK(rows[b] >= 7 && rows[b] <= T, "vfx_op_ssim: image %d has %d rows (need 7 .. T = %d)", b, rows[b], T);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const int* d_rows = upload_lens(sc.blob, rows, B);
    const int64_t stride = ssim_tiles(T, F);
    double* ws = static_cast<double*>(sc.blob.alloc((size_t)B * stride * sizeof(double)));
    launch_ssim_tiles(est, target, B, T, F, d_rows, ws, s);
    ScoreFinalArgs a;
    a.frames = d_rows;
    a.ssim_ws[0] = ws;
    a.ssim_stride[0] = stride;
    a.F[0] = F;
    score_column(a, B, 4, sc.blob, out, s);
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_sisdr(vfx_handle* h, const float* est, const float* target, int B, int L, const int* lens, double* out, void* stream) {
  try {
    VFX_CHECK(h && est && target && lens && out && B > 0 && B <= 65535 && L > 0, "vfx_op_sisdr: bad argument");
    for (int b = 0; b < B; ++b) VFX_CHECK(lens[b] >= 1 && lens[b] <= L, "vfx_op_sisdr: clip %d has %d samples (need 1 .. L = %d)", b, lens[b], L);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const int* d_lens = upload_lens(sc.blob, lens, B);
    const int nslab = sisdr_slabs(L);
    double* ws = static_cast<double*>(sc.blob.alloc((size_t)B * nslab * 3 * sizeof(double)));
    launch_sisdr_slabs(est, target, B, L, d_lens, nslab, ws, s);
    ScoreFinalArgs a;
    a.lens = d_lens;
    a.sisdr_ws = ws;
    a.nslab = nslab;
    score_column(a, B, 0, sc.blob, out, s);
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

// the scoring launches of the two scored restore entries on caller tensors: logmel == NULL: those of the SSR entry on (den, target_mel)
static int op_handler_metrics(const char* who, vfx_handle* h, const float* logmel, const float* den, const float* target_mel, int B, int T,
                              const int* frames, double* out, void* stream) {
  try {
    VFX_CHECK(h && den && target_mel && frames && out && B > 0 && B <= 65535 && T >= 7, "%s: bad argument", who);
    for (int b = 0; b < B; ++b) VFX_CHECK(frames[b] >= 7 && frames[b] <= T, "%s: clip %d has %d frames (need 7 .. T = %d)", who, b, frames[b], T);
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const int* d_frames = upload_lens(sc.blob, frames, B);
    char* ws = static_cast<char*>(sc.blob.alloc(handler_metrics_ws_bytes(B, T)));
    if (logmel) launch_handler_metrics(logmel, den, target_mel, B, T, d_frames, ws, out, s);
    else launch_mel_metrics(den, target_mel, B, T, d_frames, ws, out, s);
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_handler_metrics(vfx_handle* h, const float* logmel, const float* den, const float* target_mel, int B, int T,
                                      const int* frames, double* out, void* stream) {
  if (!logmel) {
    set_error("vfx_op_handler_metrics: bad argument");
    return 1;
  }
  return op_handler_metrics("vfx_op_handler_metrics", h, logmel, den, target_mel, B, T, frames, out, stream);
}

extern "C" int vfx_op_mel_metrics(vfx_handle* h, const float* est_mel, const float* target_mel, int B, int T, const int* frames, double* out,
                                  void* stream) {
  return op_handler_metrics("vfx_op_mel_metrics", h, nullptr, est_mel, target_mel, B, T, frames, out, stream);
}

extern "C" int vfx_op_score_spectrogram(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, int rate, float* sp,
                                        float* mel, void* stream) {
  try {
    VFX_CHECK(h && wav && lengths && sp && mel && B > 0 && B <= 65535 && Lmax > 0, "vfx_op_score_spectrogram: bad argument");
    VFX_CHECK(rate == 44100 || rate == kDftRate, "vfx_op_score_spectrogram: rate %d is not scored (the supported rates are 44100 and 16000)",
              rate);
    const int min_len = rate == kDftRate ? kDftMinLen : 6 * h->cfg.hop;
    VFX_CHECK(rate == kDftRate ? Lmax < (1 << 30) : h->cfg.n_fft == 2048 && h->cfg.n_mels == 128,
              "vfx_op_score_spectrogram: Lmax too long, or not the 44.1 kHz front end");
    int T = 0;
    for (int b = 0; b < B; ++b) {
      VFX_CHECK(lengths[b] >= min_len && lengths[b] <= Lmax, "vfx_op_score_spectrogram: clip %d has %d samples (need %d <= length <= Lmax = %d)",
                b, lengths[b], min_len, Lmax);
      T = std::max(T, rate == kDftRate ? dft_frames(lengths[b]) : lengths[b] / h->cfg.hop + 1);
    }
    DeviceGuard device_guard_(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc;
    const int* d_lens = upload_lens(sc.blob, lengths, B);
    if (rate == kDftRate)
      launch_stft_dft(ensure_score16k_tables(h), wav, B, Lmax, T, d_lens, sp, mel, s);
    else
      launch_stft_mel(h->fe, wav, B, Lmax, T, mel, sp, nullptr, nullptr, 0, h->cfg.hop, 0.f, s, d_lens);
    VFX_HIP(hipStreamSynchronize(s));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_stoi_stage(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lens, int up, int down,
                                 const double* taps, int ntaps, int stage, double* out, int64_t out_n, int* iout, int64_t iout_n,
                                 void* stream) {
  try {
    VFX_CHECK(h != nullptr, "vfx_op_stoi_stage: NULL handle");
    DeviceGuard device_guard_(h->device);
    StoiStageOut so;
    so.stage = stage;
    so.out = out;
    so.out_n = out_n;
    so.iout = iout;
    so.iout_n = iout_n;
    Scratch sc;
    double* scores = static_cast<double*>(sc.blob.alloc((size_t)std::max(B, 1) * sizeof(double)));
    stoi_scores(h, est, target, B, Lmax, lens, up, down, taps, ntaps, scores, &so, static_cast<hipStream_t>(stream));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}

extern "C" int vfx_op_bsseval_stage(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lens, int flen,
                                    int stage, double* out, int64_t out_n, void* stream) {
  try {
    VFX_CHECK(h != nullptr, "vfx_op_bsseval_stage: NULL handle");
    DeviceGuard device_guard_(h->device);
    BssStageOut so;
    so.stage = stage;
    so.out = out;
    so.out_n = out_n;
    Scratch sc;
    double* scores = static_cast<double*>(sc.blob.alloc((size_t)std::max(B, 1) * 3 * sizeof(double)));
    bsseval_scores(h, est, target, B, Lmax, lens, flen, scores, &so, static_cast<hipStream_t>(stream));
  } catch (const vfx::Error&) {
    return 1;
  }
  return 0;
}
