// resunet.cpp -- weights and launch plans of the two ResUNets.
//
//   mel ResUNet          models/components/unet.py:12-103     (B,1,T,128) log-mel -> residual
//   spectrogram ResUNet  models/components/unet_v2.py:21-148  (B,1,T,1025) magnitude -> magnitude
//
// Both share the trunk: 6 x EncoderBlockRes4B (modules.py:167-184), ConvBlockRes bottleneck,
// 6 x DecoderBlockRes4B (modules.py:186-220), after_conv_block1, after_conv2.  Activations live
// in the workspace arena as channels-last fp32 (B, H=T, W=F, C).  Every 3x3 / 1x1 / transposed
// convolution with Cin >= 32 is one launch (4 for a transposed conv) of the tap-convolution
// kernel; BatchNorm (eval mode) is folded into a per-channel affine applied, together with the
// LeakyReLU, while the input tile is staged into LDS; the residual add / 1x1 shortcut / channel
// concat never materialise.
#include <cmath>

#include "vfx_internal.h"

namespace vfx {

static const int kEncC[6] = {32, 64, 128, 256, 384, 384};                  // unet.py:22-33
static const int kDecIn[6] = {384, 384, 384, 256, 128, 64};                // unet.py:36-47
static const int kDecOut[6] = {384, 384, 256, 128, 64, 32};
static const float kBnEps = 1e-5f;
static const float kSlope = 0.01f;  // modules.py:265-266

namespace {

struct Staged {
  vfx_handle* h;
  int model;
  const HostTensor& get(const std::string& name) const {
    auto it = h->staged[model].find(name);
    VFX_CHECK(it != h->staged[model].end(), "missing tensor '%s' for model %d", name.c_str(), model);
    return it->second;
  }
  bool has(const std::string& name) const { return h->staged[model].count(name) != 0; }
};

std::vector<std::pair<int, int>> taps3x3() {
  std::vector<std::pair<int, int>> t;
  for (int kh = 0; kh < 3; ++kh)
    for (int kw = 0; kw < 3; ++kw) t.push_back({kh, kw});
  return t;
}

// eval-mode BatchNorm2d -> (scale, shift)
void fold_bn(const Staged& st, const std::string& p, int n, std::vector<float>& scale, std::vector<float>& shift) {
  const HostTensor &g = st.get(p + ".weight"), &b = st.get(p + ".bias"), &m = st.get(p + ".running_mean"),
                   &v = st.get(p + ".running_var");
  VFX_CHECK((int)g.data.size() == n && (int)v.data.size() == n, "%s: expected %d features", p.c_str(), n);
  scale.resize(n);
  shift.resize(n);
  for (int i = 0; i < n; ++i) {
    const float s = g.data[i] / std::sqrt(v.data[i] + kBnEps);
    scale[i] = s;
    shift[i] = b.data[i] - m.data[i] * s;
  }
}

void check_shape(const HostTensor& t, std::initializer_list<int64_t> shp, const std::string& name) {
  VFX_CHECK(t.shape == std::vector<int64_t>(shp), "tensor '%s' has an unexpected shape", name.c_str());
}

ConvBlockW block_shape(int cin, int cout, int nsrc) {
  ConvBlockW w;
  w.cin = cin;
  w.cout = cout;
  w.nsrc = nsrc;
  w.shortcut = cin != cout;
  return w;
}

// `w` comes with its channel counts (unet_weight_shapes); the tensors of block `p` are checked against them, packed and uploaded
void load_block(const Staged& st, DeviceBlob& blob, const std::string& p, ConvBlockW& w) {
  const bool split = st.h->cfg.precision != 0;
  const int cin = w.cin, cout = w.cout, nsrc = w.nsrc;
  std::vector<float> sc, sh;
  fold_bn(st, p + ".bn1", cin, sc, sh);
  w.bn1_scale = blob.upload(sc);
  w.bn1_shift = blob.upload(sh);
  fold_bn(st, p + ".bn2", cout, sc, sh);
  w.bn2_scale = blob.upload(sc);
  w.bn2_shift = blob.upload(sh);
  const HostTensor& c1 = st.get(p + ".conv1.weight");
  check_shape(c1, {cout, cin, 3, 3}, p + ".conv1.weight");
  const HostTensor& c2 = st.get(p + ".conv2.weight");
  check_shape(c2, {cout, cout, 3, 3}, p + ".conv2.weight");
  const int cs = cin / nsrc;
  if (cin >= kKC)
    for (int s = 0; s < nsrc; ++s) w.w1[s] = blob.upload(pack_conv(c1.data.data(), cout, cin, 3, 3, s * cs, cs, taps3x3(), split));
  w.w2 = blob.upload(pack_conv(c2.data.data(), cout, cout, 3, 3, 0, cout, taps3x3(), split));
  VFX_CHECK(w.shortcut == st.has(p + ".shortcut.weight"), "%s: shortcut presence does not match channel counts", p.c_str());
  if (w.shortcut) {
    const HostTensor& ws = st.get(p + ".shortcut.weight");
    check_shape(ws, {cout, cin, 1, 1}, p + ".shortcut.weight");
    if (cin >= kKC)
      for (int s = 0; s < nsrc; ++s)
        w.wsc[s] = blob.upload(pack_conv(ws.data.data(), cout, cin, 1, 1, s * cs, cs, {{0, 0}}, split));
    w.bsc = blob.upload(st.get(p + ".shortcut.bias").data);
  }
}

}  // namespace

UNetWeights unet_weight_shapes() {
  UNetWeights W;
  int cin = 1;
  for (int l = 0; l < 6; ++l) {
    const int c = kEncC[l];
    for (int j = 0; j < 4; ++j) W.enc[l][j] = block_shape(j == 0 ? cin : c, c, 1);
    cin = c;
  }
  W.bott = block_shape(384, 384, 1);
  for (int d = 0; d < 6; ++d) {
    DecoderW& D = W.dec[d];
    D.cin = kDecIn[d];
    D.cout = kDecOut[d];
    for (int j = 0; j < 4; ++j) D.blocks[j] = block_shape(j == 0 ? 2 * D.cout : D.cout, D.cout, j == 0 ? 2 : 1);
  }
  W.after = block_shape(32, 32, 1);
  return W;
}

std::shared_ptr<UNetWeights> build_unet_weights(vfx_handle* h, int model) {
  Staged st{h, model};
  auto W = std::make_shared<UNetWeights>(unet_weight_shapes());
  DeviceBlob& blob = h->blob;
  for (int l = 0; l < 6; ++l) {
    char p[64];
    for (int j = 0; j < 4; ++j) {
      snprintf(p, sizeof(p), "encoder_block%d.conv_block%d", l + 1, j + 1);
      load_block(st, blob, p, W->enc[l][j]);
    }
  }
  // Cin = 1 entry convs of encoder_block1.conv_block1
  {
    const std::string p = "encoder_block1.conv_block1";
    std::vector<float> sc, sh;
    fold_bn(st, p + ".bn1", 1, sc, sh);
    W->c1_scale = sc[0];
    W->c1_shift = sh[0];
    const HostTensor& c1 = st.get(p + ".conv1.weight");  // (32,1,3,3) -> [tap][32]
    std::vector<float> w(9 * 32);
    for (int n = 0; n < 32; ++n)
      for (int t = 0; t < 9; ++t) w[t * 32 + n] = c1.data[n * 9 + t];
    W->c1_w = blob.upload(w);
    W->c1_wsc = blob.upload(st.get(p + ".shortcut.weight").data);  // (32,1,1,1)
    W->c1_bsc = blob.upload(st.get(p + ".shortcut.bias").data);
  }
  load_block(st, blob, "conv_block7", W->bott);
  for (int d = 0; d < 6; ++d) {
    DecoderW& D = W->dec[d];
    char p[64];
    snprintf(p, sizeof(p), "decoder_block%d", d + 1);
    std::vector<float> sc, sh;
    fold_bn(st, std::string(p) + ".bn1", D.cin, sc, sh);
    D.bn_scale = blob.upload(sc);
    D.bn_shift = blob.upload(sh);
    const HostTensor& wt = st.get(std::string(p) + ".conv1.weight");
    check_shape(wt, {D.cin, D.cout, 3, 3}, std::string(p) + ".conv1.weight");
    // output parity class (a, b) = (oh & 1, ow & 1): kernel rows kh == a (mod 2), cols kw == b (mod 2)
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        std::vector<std::pair<int, int>> taps;
        for (int kh = a; kh < 3; kh += 2)
          for (int kw = b; kw < 3; kw += 2) taps.push_back({kh, kw});
        D.wT[a * 2 + b] = blob.upload(pack_conv_transposed(wt.data.data(), D.cin, D.cout, 3, 3, taps, h->cfg.precision != 0));
      }
    for (int j = 0; j < 4; ++j) {
      char q[96];
      snprintf(q, sizeof(q), "%s.conv_block%d", p, j + 2);
      load_block(st, blob, q, D.blocks[j]);
    }
  }
  load_block(st, blob, "after_conv_block1", W->after);
  const HostTensor& fw = st.get("after_conv2.weight");
  check_shape(fw, {1, 32, 1, 1}, "after_conv2.weight");
  W->final_w = blob.upload(fw.data);
  W->final_b = st.get("after_conv2.bias").data[0];
  return W;
}

// ---------------------------------------------------------------------------------------------
// plan construction
// ---------------------------------------------------------------------------------------------
// ConvTranspose2d(k3, s2, p0) + prune on (B, H, W, Cin) -> (B, 2H, 2W [+ 1], Cout) as tap convolutions: output parity class
// (a, b) = (oh & 1, ow & 1) is a convolution with the kernel rows kh == a and columns kw == b (mod 2), weights wT[2 a + b].
// Three forms, the same stage tables and sums in each (bit-identical):
//   * ONE launch of four phases r = 2 a + b, for either output width: the output is addressed in units of Cout channels at the TRUE
//     pixel index (TapConvParams::out_cmul: phase r lands at column 2 j + (r & 1)), phases 2 and 3 write the odd output rows
//     (TapConvParams::phase_rows), and a block of k_conv covers up to four phases: the patch is staged once and x read from HBM once.
//   * VFX_TUNE_TWO_LAUNCH_UPSAMPLERS: one launch per output row class, its two column classes the phases.  An even output width makes
//     (B, 2H, 2W, C) a (B, 2H, W, 2C) tensor whose channel halves are the column parities; an odd one (2 W + 1: the mel ResUNet prunes
//     the time axis only) has no such view and is addressed through out_cmul, column class 1 one column short.
//   * four launches, one per parity class: an image of one row or column (plan_conv finds a tile whose all-taps window fits one patch,
//     which a phased launch needs, from 2 x 2 up), VFX_TUNE_NO_FUSED_UNET, a bias, or couts that are no multiple of 32.
std::vector<ConvLaunch> unet_upsample_launches(int tuning, int B, int H, int W, int Cin, int Cout, bool prune_w, const float* src, float* out,
                                               const float* scale, const float* shift, int act, float slope, const float* const wT[4],
                                               const float* bias) {
  const int Ho = 2 * H, Wo = prune_w ? 2 * W : 2 * W + 1;
  const bool phased = H >= 2 && W >= 2 && !(tuning & VFX_TUNE_NO_FUSED_UNET) && !bias && Cout % 32 == 0;
#ifdef VFX_ABL_NO_ODD_PHASED  // (measurement builds: four launches at an odd width)
  const bool two_ok = phased && prune_w;
#else
  const bool two_ok = phased;
#endif
  const bool four = phased && !(tuning & VFX_TUNE_TWO_LAUNCH_UPSAMPLERS);
  const int na = four ? 2 : 1, nb = (four || two_ok) ? 2 : 1;  // row and column classes per launch
  std::vector<ConvLaunch> launches;
  for (int a0 = 0; a0 < 2; a0 += na)
    for (int b0 = 0; b0 < 2; b0 += nb) {
      ConvLaunch l{};
      TapConvParams& p = l.p;
      p.B = B;
      p.Hi = H;
      p.Wi = W;
      p.Ho = Ho;
      p.Wo = Wo;
      p.Cout = na * nb * Cout;
      p.sh = p.sw = 2;
      p.oh0 = a0;
      p.ow0 = b0;
      p.Hg = (Ho - a0 + 1) / 2;  // (row class 1 has Ho / 2 rows; beside class 0 in one launch: masked, oh < Ho)
      p.Wg = (Wo - b0 + 1) / 2;  // column class 0: W + 1 columns of an odd width, W of a pruned one; class 1 beside it masked (ow + 1 < Wo)
      if (nb == 2 && na == 1 && prune_w) {  // the (B, 2H, W, 2C) view
        p.Wo = W;
        p.sw = 1;
      } else if (nb == 2) {
        p.out_cmul = Cout;
        p.phase_rows = na == 2;
      }
      p.bias = bias;
      p.out = out;
      p.act_slope = 1.f;
      p.nseg = 1;
      std::vector<TapSeg> phases;
      for (int a = a0; a < a0 + na; ++a)
        for (int b = b0; b < b0 + nb; ++b) {
          TapSeg S{};
          S.src = src;
          S.C = Cin;
          S.scale = scale;
          S.shift = shift;
          S.act = act;
          S.slope = slope;
          S.wt = wT[a * 2 + b];
          for (int kh = a; kh < 3; kh += 2)
            for (int kw = b; kw < 3; kw += 2) {
              S.dh[S.ntaps] = -(kh / 2);  // oh = 2*ih + kh  ->  ih = i - kh/2 for oh = 2i + a
              S.dw[S.ntaps] = -(kw / 2);
              ++S.ntaps;
            }
          phases.push_back(S);
        }
      p.seg[0] = phases[0];  // the launch's first class reads the kernel rows / columns {0, 2} its others lack: the union of their windows
      if (phases.size() > 1) l.phases = phases;
      launches.push_back(l);
    }
  return launches;
}

namespace {

struct Act4 {  // an activation tensor in the arena
  size_t off = 0;
  int H = 0, W = 0, C = 0;
};

struct TrunkBuilder {
  PlanBuilder& pb;
  const UNetWeights& Wt;
  int B;

  Act4 make(int H, int W, int C) {
    Act4 a;
    a.H = H;
    a.W = W;
    a.C = C;
    a.off = pb.alloc_f((int64_t)B * H * W * C);
    return a;
  }

  static void set_taps3x3(TapSeg& s) {
    s.ntaps = 9;
    for (int kh = 0; kh < 3; ++kh)
      for (int kw = 0; kw < 3; ++kw) {
        s.dh[kh * 3 + kw] = kh - 1;
        s.dw[kh * 3 + kw] = kw - 1;
      }
  }

  TapConvParams base(const Act4& geo, int Cout, size_t out_off) {
    TapConvParams p{};
    p.B = B;
    p.Hi = p.Hg = p.Ho = geo.H;
    p.Wi = p.Wg = p.Wo = geo.W;
    p.Cout = Cout;
    p.sh = p.sw = 1;
    p.act_slope = 1.f;
    p.out = const_cast<float*>(rel_ptr(out_off));
    return p;
  }

  // y = ConvBlockRes(x) where x = cat(srcs) (1 or 2 sources); frees nothing.
  // `pre_h` / `pre_sc`: first block of the network, conv1 and shortcut already computed (Cin = 1).
  // `h_out` (build_unet_piece): receives the two-launch form's intermediate tensor (C = 0: one launch, h never leaves LDS).
  Act4 conv_block(const ConvBlockW& w, const Act4* srcs, int nsrc, const Act4* pre_h = nullptr,
                  const Act4* pre_sc = nullptr, Act4* h_out = nullptr) {
    const Act4& g = srcs ? srcs[0] : *pre_h;
    // Identity-shortcut blocks of the C = 32 / 64 levels run as ONE launch of k_resblock's 2-D mode: h stays in LDS, 402
    // instead of 872 HBM bytes per output pixel (VFX_TUNE_NO_FUSED_UNET: the two-launch form).
    const bool fuse2d = !(pb.h->cfg.tuning & VFX_TUNE_NO_FUSED_UNET);
    if (fuse2d && srcs && nsrc == 1 && !w.shortcut && !pre_h && block2d_supported(w.cout) && pb.h->cfg.precision != 0) {
      Act4 y = make(g.H, g.W, w.cout);
      ResBlockParams rp{};
      rp.geo2d = 1;
      rp.x = rel_ptr(srcs[0].off);
      rp.y = const_cast<float*>(rel_ptr(y.off));
      rp.w1 = w.w1[0];
      rp.w2 = w.w2;
      rp.sc1 = w.bn1_scale;
      rp.sh1 = w.bn1_shift;
      rp.sc2 = w.bn2_scale;
      rp.sh2 = w.bn2_shift;
      rp.slope = kSlope;
      rp.B = B;
      rp.H = g.H;
      rp.W = g.W;
      rp.C = w.cout;
      pb.add_resblock(rp);
      return y;
    }
    // The two-source block with a 1x1 shortcut at C = 32 (decoder_block6.conv_block2): one launch too (resblock.hip, SC2)
#ifndef VFX_ABL_NO_SC2
    if (fuse2d && srcs && nsrc == 2 && w.shortcut && w.cout == 32 && srcs[0].C == 32 && srcs[1].C == 32 &&
        pb.h->cfg.precision != 0 && !(pb.h->cfg.tuning & VFX_TUNE_SMALL_2D_TILES)) {
      Act4 y = make(g.H, g.W, w.cout);
      ResBlockParams rp{};
      rp.geo2d = 1;
      rp.two_src = 1;
      rp.x = rel_ptr(srcs[0].off);
      rp.x2 = rel_ptr(srcs[1].off);
      rp.y = const_cast<float*>(rel_ptr(y.off));
      rp.w1 = w.w1[0];
      rp.w1x2 = w.w1[1];
      rp.w2 = w.w2;
      rp.wsc = w.wsc[0];
      rp.wsc2 = w.wsc[1];
      rp.bsc = w.bsc;
      rp.sc1 = w.bn1_scale;
      rp.sh1 = w.bn1_shift;
      rp.sc2 = w.bn2_scale;
      rp.sh2 = w.bn2_shift;
      rp.slope = kSlope;
      rp.B = B;
      rp.H = g.H;
      rp.W = g.W;
      rp.C = w.cout;
      pb.add_resblock(rp);
      return y;
    }
#endif
    Act4 hbuf;
    if (pre_h) {
      hbuf = *pre_h;
    } else {
      hbuf = make(g.H, g.W, w.cout);
      TapConvParams p = base(g, w.cout, hbuf.off);
      p.nseg = nsrc;
      int coff = 0;
      for (int s = 0; s < nsrc; ++s) {
        TapSeg& S = p.seg[s];
        S.src = rel_ptr(srcs[s].off);
        S.C = srcs[s].C;
        S.scale = w.bn1_scale + coff;
        S.shift = w.bn1_shift + coff;
        S.act = ACT_LEAKY;
        S.slope = kSlope;
        S.wt = w.w1[s];
        set_taps3x3(S);
        coff += srcs[s].C;
      }
      // h feeds conv2 only: store it ACTIVATED (bn2 affine + LeakyReLU applied once per element, operand form)
      p.out_act = p.out;
      p.out = nullptr;
      p.act_scale = w.bn2_scale;
      p.act_shift = w.bn2_shift;
      p.act_slope = kSlope;
      pb.add_conv(p);
    }
    Act4 y = make(g.H, g.W, w.cout);
    TapConvParams p = base(g, w.cout, y.off);
    TapSeg& S0 = p.seg[0];
    S0.src = rel_ptr(hbuf.off);
    S0.C = w.cout;
    if (pre_h) {  // h of the Cin = 1 entry block comes raw from k_conv_c1
      S0.scale = w.bn2_scale;
      S0.shift = w.bn2_shift;
      S0.act = ACT_LEAKY;
      S0.slope = kSlope;
    } else {
      S0.src_act = 1;
      S0.act = ACT_NONE;
      S0.slope = 1.f;
    }
    S0.wt = w.w2;
    set_taps3x3(S0);
    p.nseg = 1;
    if (pre_sc) {
      p.residual = rel_ptr(pre_sc->off);  // shortcut(x) incl. bias, computed by the Cin=1 kernel
    } else if (w.shortcut) {
      for (int s = 0; s < nsrc; ++s) {
        TapSeg& S = p.seg[p.nseg++];
        S.src = rel_ptr(srcs[s].off);
        S.C = srcs[s].C;
        S.scale = nullptr;
        S.shift = nullptr;
        S.act = ACT_NONE;
        S.slope = 1.f;
        S.wt = w.wsc[s];
        S.ntaps = 1;
        S.dh[0] = 0;
        S.dw[0] = 0;
      }
      p.bias = w.bsc;
    } else {
      p.residual = rel_ptr(srcs[0].off);
    }
    pb.add_conv(p);
    if (h_out) *h_out = hbuf;
    if (!pre_h) pb.free(hbuf.off);
    return y;
  }

  Act4 pool(const Act4& x) {
    Act4 y = make(x.H / 2, x.W / 2, x.C);
    Plan* pl = pb.plan;
    const int Bc = B;
    const Act4 xi = x;
    const size_t yo = y.off;
    pl->ops.push_back([=](const RunCtx& c) {
      launch_avgpool2(reinterpret_cast<const float*>(pl->bound_base + xi.off), Bc, xi.H, xi.W, xi.C,
                      reinterpret_cast<float*>(pl->bound_base + yo), c.stream);
    });
    return y;
  }

  // BN -> ReLU -> ConvTranspose2d(k3, s2, p0) -> prune (modules.py:205-214)
  Act4 upsample(const DecoderW& D, const Act4& x, bool prune_w) {
    Act4 y = make(2 * x.H, prune_w ? 2 * x.W : 2 * x.W + 1, D.cout);
    for (const ConvLaunch& l : unet_upsample_launches(pb.h->cfg.tuning, B, x.H, x.W, x.C, D.cout, prune_w, rel_ptr(x.off),
                                                      const_cast<float*>(rel_ptr(y.off)), D.bn_scale, D.bn_shift, ACT_LEAKY, 0.f /* ReLU */,
                                                      D.wT, nullptr))
      pb.add_conv(l);
    return y;
  }

  // encoder_block1.conv_block1 (Cin = 1) on the single-channel plane at x_off: one launch of the fused block's entry form
  // (resblock.hip, IN1), or -- fp32 mode, VFX_TUNE_NO_FUSED_UNET / VFX_TUNE_SMALL_2D_TILES -- k_conv_c1 (conv1 and the shortcut) +
  // k_conv (conv2).  `h_out` (build_unet_piece): k_conv_c1's raw conv1 output of the two-launch form (C = 0: one launch).
  Act4 entry(size_t x_off, int H, int W0, Act4* h_out = nullptr) {
    Plan* pl = pb.plan;
    const UNetWeights* wp = &Wt;
    const int Bc = B;
    const int tun = pb.h->cfg.tuning;
#ifdef VFX_ABL_NO_IN1  // measurement builds (scripts/build_variant.sh)
    const bool entry_fused = false;
#else
    const bool entry_fused = !(tun & (VFX_TUNE_NO_FUSED_UNET | VFX_TUNE_SMALL_2D_TILES)) && pb.h->cfg.precision != 0;
#endif
    if (entry_fused) {
      Act4 y = make(H, W0, 32);
      const ConvBlockW& w = Wt.enc[0][0];
      ResBlockParams rp{};
      rp.geo2d = 1;
      rp.in1 = 1;
      rp.x = rel_ptr(x_off);
      rp.y = const_cast<float*>(rel_ptr(y.off));
      rp.w1 = Wt.c1_w;
      rp.w2 = w.w2;
      rp.in1_scale = Wt.c1_scale;
      rp.in1_shift = Wt.c1_shift;
      rp.wsc = Wt.c1_wsc;
      rp.bsc = Wt.c1_bsc;
      rp.sc2 = w.bn2_scale;
      rp.sh2 = w.bn2_shift;
      rp.slope = kSlope;
      rp.B = B;
      rp.H = H;
      rp.W = W0;
      rp.C = 32;
      pb.add_resblock(rp);
      return y;
    }
    Act4 h1 = make(H, W0, 32), sc1 = make(H, W0, 32);
    {
      const size_t ho = h1.off, so = sc1.off;
      pl->ops.push_back([=](const RunCtx& c) {
        launch_conv_c1(reinterpret_cast<const float*>(pl->bound_base + x_off), Bc, H, W0, wp->c1_w, wp->c1_scale,
                       wp->c1_shift, kSlope, wp->c1_wsc, wp->c1_bsc, reinterpret_cast<float*>(pl->bound_base + ho),
                       reinterpret_cast<float*>(pl->bound_base + so), c.stream);
      });
    }
    Act4 y = conv_block(Wt.enc[0][0], nullptr, 0, &h1, &sc1, h_out);
    pb.free(h1.off);
    pb.free(sc1.off);
    return y;
  }

  // Whole trunk from the single-channel input plane x1 (B, Tpad, W0) to the 32-channel tensor
  // in front of after_conv2.
  Act4 run(size_t x_off, int Tpad, int W0, bool both) {
    Act4 skips[6];
    Act4 y = entry(x_off, Tpad, W0);
    for (int l = 0; l < 6; ++l) {
      for (int j = (l == 0 ? 1 : 0); j < 4; ++j) {
        Act4 y2 = conv_block(Wt.enc[l][j], &y, 1);
        pb.free(y.off);
        y = y2;
      }
      skips[l] = y;
      y = pool(y);
    }
    {
      Act4 y2 = conv_block(Wt.bott, &y, 1);
      pb.free(y.off);
      y = y2;
    }
    for (int d = 0; d < 6; ++d) {
      const DecoderW& D = Wt.dec[d];
      const Act4& skip = skips[5 - d];
      Act4 up = upsample(D, y, both);
      pb.free(y.off);
      VFX_CHECK(up.H == skip.H && up.W == skip.W, "decoder %d: upsampled %dx%d vs skip %dx%d", d + 1, up.H, up.W, skip.H,
                skip.W);
      Act4 srcs[2] = {up, skip};
      y = conv_block(D.blocks[0], srcs, 2);
      pb.free(up.off);
      pb.free(skip.off);
      for (int j = 1; j < 4; ++j) {
        Act4 y2 = conv_block(D.blocks[j], &y, 1);
        pb.free(y.off);
        y = y2;
      }
    }
    Act4 y2 = conv_block(Wt.after, &y, 1);
    pb.free(y.off);
    return y2;
  }
};

float* resolve(const Plan* pl, const RunCtx& c, const BufRef& b) {
  return b.ext ? c.ext[b.slot] : reinterpret_cast<float*>(pl->bound_base + b.off);
}

// The launches in front of and behind the trunk, as build_unet_mel / build_unet_spec and build_unet_piece append them.
// A varlen batch (PlanBuilder::lens_t): every clip has its own frame count inside the SAME padded length -- the rows past it are
// zeros like the network's own time padding (unet.py:75-77), so the trunk computes for each clip what its batch-of-one call
// computes; no kernel of the trunk needs to know.
void add_prep_logmel(PlanBuilder& pb, int B, int T, int Tpad, BufRef mel_linear, size_t x_off) {
  Plan* pl = pb.plan;
  const int* lens_t = pb.lens_t;
  pl->ops.push_back([=](const RunCtx& c) {
    launch_prep_logmel(resolve(pl, c, mel_linear), B, T, Tpad, reinterpret_cast<float*>(pl->bound_base + x_off), c.flags,
                       c.stream, lens_t);
  });
}
void add_prep_spec(PlanBuilder& pb, int B, int T, int Tpad, BufRef sp, size_t x_off) {
  Plan* pl = pb.plan;
  const int* lens_t = pb.lens_t;
  pl->ops.push_back([=](const RunCtx& c) {
    launch_prep_spec(resolve(pl, c, sp), B, T, Tpad, reinterpret_cast<float*>(pl->bound_base + x_off), c.stream, lens_t);
  });
}
// mode 0: aux0 = the linear mel, out0 = the log-mel estimate; mode 1: aux0 / aux1 = cos / sin, out0 / out1 = re / im
void add_final(PlanBuilder& pb, const UNetWeights& Wt, int B, int Tpad, int W0, int mode, int T, size_t y_off, BufRef aux0, BufRef aux1,
               BufRef out0, BufRef out1) {
  Plan* pl = pb.plan;
  const UNetWeights* wp = &Wt;
  pl->ops.push_back([=](const RunCtx& c) {
    launch_final_1x1(reinterpret_cast<const float*>(pl->bound_base + y_off), B, Tpad, W0, wp->final_w, wp->final_b, mode, T,
                     resolve(pl, c, aux0), mode ? resolve(pl, c, aux1) : nullptr, resolve(pl, c, out0),
                     mode ? resolve(pl, c, out1) : nullptr, c.stream);
  });
}

}  // namespace

void build_unet_mel(PlanBuilder& pb, int B, int T, BufRef mel_linear, BufRef logmel_out) {
  VFX_CHECK(pb.h->unet[VFX_MODEL_UNET_MEL], "mel ResUNet weights are not finalized");
  const UNetWeights& Wt = *pb.h->unet[VFX_MODEL_UNET_MEL];
  const int Tpad = (T + 63) / 64 * 64, W0 = 127;
  pb.short_clip = Tpad <= 128 ? 1 : (Tpad >= 2048 ? -(Tpad / 1024) : 0);  // split-K rule of the deep levels (TapConvParams::short_clip)
  const size_t x_off = pb.alloc_f((int64_t)B * Tpad * W0);
  add_prep_logmel(pb, B, T, Tpad, mel_linear, x_off);
  TrunkBuilder tb{pb, Wt, B};
  Act4 y = tb.run(x_off, Tpad, W0, /*both=*/false);
  pb.free(x_off);
  add_final(pb, Wt, B, Tpad, W0, 0, T, y.off, mel_linear, BufRef{}, logmel_out, BufRef{});
  pb.free(y.off);
}

void build_unet_spec(PlanBuilder& pb, int B, int T, BufRef sp, BufRef cosb, BufRef sinb, BufRef re_out, BufRef im_out) {
  VFX_CHECK(pb.h->unet[VFX_MODEL_UNET_SPEC], "spectrogram ResUNet weights are not finalized");
  const UNetWeights& Wt = *pb.h->unet[VFX_MODEL_UNET_SPEC];
  const int Tpad = (T + 63) / 64 * 64, W0 = 1024;
  pb.short_clip = Tpad <= 128 ? 1 : (Tpad >= 2048 ? -(Tpad / 1024) : 0);  // split-K rule of the deep levels (TapConvParams::short_clip)
  const size_t x_off = pb.alloc_f((int64_t)B * Tpad * W0);
  add_prep_spec(pb, B, T, Tpad, sp, x_off);
  TrunkBuilder tb{pb, Wt, B};
  Act4 y = tb.run(x_off, Tpad, W0, /*both=*/true);
  pb.free(x_off);
  add_final(pb, Wt, B, Tpad, W0, 1, T, y.off, cosb, sinb, re_out, im_out);
  pb.free(y.off);
}

// One piece of the plans above on its own (vfx_internal.h, UNetPiece): the SAME member functions TrunkBuilder::run calls and the same
// add_prep_* / add_final, over buffers of the piece's own in the arena.
void build_unet_piece(PlanBuilder& pb, const UNetWeights& Wt, UNetPiece& pc) {
  const std::string name = pc.name ? pc.name : "";
  const int B = pc.B, H = pc.H, W = pc.W;
  VFX_CHECK(B > 0 && H > 0 && W > 0, "unet piece: bad shape");
  TrunkBuilder tb{pb, Wt, B};
  pc.nin = pc.nout = 0;
  pc.h_n = 0;
  pc.h_form = 0;
  auto input = [&](int h, int w, int c) {
    Act4 a = tb.make(h, w, c);
    pc.in_off[pc.nin] = a.off;
    pc.in_n[pc.nin++] = (int64_t)B * h * w * c;
    return a;
  };
  auto output = [&](const Act4& a) {
    pc.out_off[pc.nout] = a.off;
    pc.out_n[pc.nout++] = (int64_t)B * a.H * a.W * a.C;
  };
  auto intermediate = [&](const Act4& hb, int form) {
    if (hb.C == 0) return;
    pc.h_off = hb.off;
    pc.h_n = (int64_t)B * hb.H * hb.W * hb.C;
    pc.h_form = form;
  };
  auto block = [&](const ConvBlockW& w) {
    Act4 srcs[2], hb;
    for (int s = 0; s < w.nsrc; ++s) srcs[s] = input(H, W, w.cin / w.nsrc);
    output(tb.conv_block(w, srcs, w.nsrc, nullptr, nullptr, &hb));
    intermediate(hb, 1);
  };
  int l = 0, j = 0;
  char extra = 0;
  if (name == "entry") {
    Act4 x = input(H, W, 1), hb;
    output(tb.entry(x.off, H, W, &hb));
    intermediate(hb, 0);
  } else if (name == "bott") {
    block(Wt.bott);
  } else if (name == "after") {
    block(Wt.after);
  } else if (sscanf(name.c_str(), "enc%d.%d%c", &l, &j, &extra) == 2 && l >= 1 && l <= 6 && j >= 1 && j <= 4 && !(l == 1 && j == 1)) {
    block(Wt.enc[l - 1][j - 1]);
  } else if (sscanf(name.c_str(), "dec%d.%d%c", &l, &j, &extra) == 2 && l >= 1 && l <= 6 && j >= 1 && j <= 4) {
    block(Wt.dec[l - 1].blocks[j - 1]);
  } else if (sscanf(name.c_str(), "dec%d.u%c", &l, &extra) == 2 && extra == 'p' && name.size() == 7 && l >= 1 && l <= 6) {
    const DecoderW& D = Wt.dec[l - 1];
    output(tb.upsample(D, input(H, W, D.cin), pc.arg != 0));
  } else if (name == "pool") {
    VFX_CHECK(pc.arg > 0 && pc.arg % 4 == 0 && H >= 2 && W >= 2, "unet piece: pool needs C %% 4 == 0 and an image of 2 x 2 or more");
    output(tb.pool(input(H, W, pc.arg)));
  } else if (name == "prep_logmel" || name == "prep_spec") {  // H = T frames; W is the model's own
    const bool mel = name == "prep_logmel";
    const int T = H, Tpad = (T + 63) / 64 * 64, W0 = mel ? 127 : 1024;
    Act4 in = input(T, W0 + 1, 1);
    Act4 x = tb.make(Tpad, W0, 1);
    BufRef src;
    src.off = in.off;
    if (mel) add_prep_logmel(pb, B, T, Tpad, src, x.off);
    else add_prep_spec(pb, B, T, Tpad, src, x.off);
    output(x);
  } else if (name == "final") {  // H = T frames, W = the trunk's width; arg = mode
    const int T = H, Tpad = (T + 63) / 64 * 64, mode = pc.arg;
    VFX_CHECK(mode == 0 || mode == 1, "unet piece: final has modes 0 and 1");
    Act4 y = input(Tpad, W, 32);
    BufRef aux[2], out[2];
    for (int k = 0; k <= mode; ++k) aux[k].off = input(T, W + 1, 1).off;
    for (int k = 0; k <= mode; ++k) {
      Act4 o = tb.make(T, W + 1, 1);
      out[k].off = o.off;
      output(o);
    }
    add_final(pb, Wt, B, Tpad, W, mode, T, y.off, aux[0], aux[1], out[0], out[1]);
  } else {
    VFX_CHECK(false, "unet piece: unknown piece '%s'", name.c_str());
  }
}

// family, ksplit, activated output, bias, segments, output channels of every launch of `plan` (kUNetLaunchInts each); the plans of
// build_unet_piece run their small kernels first, then their fused blocks or convolutions
int describe_unet_launches(const Plan& plan, int* out, int cap) {
  int n = 0;
  auto put = [&](int fam, int ks, int act, int bias, int nseg, int cout) {
    if (out && (n + 1) * kUNetLaunchInts <= cap) {
      const int v[kUNetLaunchInts] = {fam, ks, act, bias, nseg, cout};
      std::copy(v, v + kUNetLaunchInts, out + n * kUNetLaunchInts);
    }
    ++n;
  };
  const size_t small = plan.ops.size() - plan.host_rb.size() - plan.host_params.size();
  for (size_t i = 0; i < small; ++i) put(UNET_LAUNCH_SMALL, 1, 0, 0, 0, 0);
  for (const ResBlockParams& q : plan.host_rb)
    put(q.in1 ? UNET_LAUNCH_BLOCK_IN1 : (q.two_src ? UNET_LAUNCH_BLOCK_TWO_SRC : (block2d32_ok(q) ? UNET_LAUNCH_BLOCK2D32 : UNET_LAUNCH_BLOCK)),
        1, 0, q.bsc != nullptr, q.two_src ? 2 : 1, q.C);
  for (const TapConvParams& q : plan.host_params)
    put(q.nphase > 1 ? UNET_LAUNCH_CONV_PHASED : UNET_LAUNCH_CONV, std::max(q.ksplit, 1), q.out_act != nullptr, q.bias != nullptr,
        q.nseg, q.Cout);
  return n;
}

}  // namespace vfx
