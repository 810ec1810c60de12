// analysis.hip -- the two non-ResUNet analysis modules of Generator (models/gsr_voicefixer.py:44-91, gfx950):
//   bi_gru: BN -> Linear 128->256 -> BN_GRU (BN + 2-layer bidirectional GRU, hidden 256) -> ReLU -> Linear 512->256 -> ReLU
//           -> Linear 256->128
//   dnn:    5 x (Linear -> ReLU [-> BN]) 128->256->512->1024->512->256, Linear 256->128
// both on x = to_log(mel) with the output analysis(x) + x.  Every BatchNorm2d(1) of eval mode is one scalar affine.
//
//   k_dense    one Linear over all M = B*T rows, fused with its input transform (to_log + negative-input flag, the scalar BN,
//              ReLU) and its epilogue (bias, ReLU, scalar BN, the + to_log(mel) residual).  fp32 FMA in every precision mode,
//              K summed in one fixed order per row: a row's result depends on nothing but that row (no split-K).
//   k_gru_seq  one GRU layer, both directions: one workgroup per (clip, direction), no inter-workgroup waits.  Thread j owns
//              gate row j of W_hh (768 x 256): its first kGruRegK columns in registers, the next kGruLdsK in LDS, the rest
//              streamed from L2 every step.  h_{t-1} lives in LDS; fp32 FMA and accurate expf / tanhf in every mode.
#include <cmath>
#include <set>

#include "conv_common.h"
#include "vfx_internal.h"

namespace vfx {

static inline unsigned nblocks_a(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------------------------------------
// k_dense: y (M, N) = epilogue(transform(x) (M, K) . wT (K, N))
// ---------------------------------------------------------------------------------------------
struct DenseArgs {
  const float* x;        // (M, K) rows; with in_log: linear mel (K = 128)
  const float* wT;       // (K, N) = the Linear's weight transposed
  const float* bias;     // (N)
  const float* resid;    // (M, N = 128) linear mel: y += to_log(resid) -- the Generator's "+ to_log(mel_orig)"; or null
  float* y;              // (M, N)
  const int* lens_t;     // frames per clip (B), or null: rows t >= lens_t[b] of a clip are zero in y and never read from x
  int* flags;
  int64_t M;
  int K, N, T;
  int in_log, in_relu, out_relu;
  float in_scale, in_shift;    // after to_log: the scalar BN of the input (1, 0 = none)
  float out_scale, out_shift;  // after ReLU: the scalar BN of the output (1, 0 = none)
};

constexpr int kDM = 64, kDN = 64, kDK = 16;

__device__ __forceinline__ float log_clip(float v) { return log10f(fmaxf(v, 1e-8f)); }

__global__ __launch_bounds__(256) void k_dense(DenseArgs a) {
  __shared__ float As[kDK][kDM + 4];
  __shared__ float Bs[kDK][kDN];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * kDM;
  const int n0 = blockIdx.y * kDN;
  // the A row this thread loads (4 consecutive k of it per K step)
  const int lr = tid >> 2, lk = (tid & 3) * 4;
  const int64_t lrow = m0 + lr;
  bool lrow_live = lrow < a.M;
  if (lrow_live && a.lens_t) {
    const int64_t b = lrow / a.T;
    lrow_live = (int)(lrow - b * a.T) < a.lens_t[b];
  }
  const float* xrow = a.x + lrow * a.K;
  const int bk = tid >> 4, bn = (tid & 15) * 4;
  bool neg = false;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int k0 = 0; k0 < a.K; k0 += kDK) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (lrow_live) {
      v = *reinterpret_cast<const f32x4*>(xrow + k0 + lk);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float e = v[i];
        if (a.in_log) {
          neg |= e < 0.f;
          e = fmaf(a.in_scale, log_clip(e), a.in_shift);
        }
        if (a.in_relu) e = fmaxf(e, 0.f);
        v[i] = e;
      }
    }
    const f32x4 w = *reinterpret_cast<const f32x4*>(a.wT + (int64_t)(k0 + bk) * a.N + n0 + bn);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) As[lk + i][lr] = v[i];
    *reinterpret_cast<f32x4*>(&Bs[bk][bn]) = w;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kDK; ++k) {
      float av[4], bv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) av[r] = As[k][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = Bs[k][tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(av[r], bv[c], acc[r][c]);
    }
  }
  if (a.in_log && __any(neg) && (tid & 63) == 0) or_flag_global(a.flags, VFX_FLAG_NEGATIVE_INPUT);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = m0 + ty + 16 * r;
    if (row >= a.M) continue;
    bool live = true;
    if (a.lens_t) {
      const int64_t b = row / a.T;
      live = (int)(row - b * a.T) < a.lens_t[b];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int n = n0 + tx + 16 * c;
      float v = 0.f;
      if (live) {
        v = acc[r][c] + a.bias[n];
        if (a.out_relu) v = fmaxf(v, 0.f);
        v = fmaf(a.out_scale, v, a.out_shift);
        if (a.resid) v += log_clip(a.resid[row * a.N + n]);
      }
      a.y[row * a.N + n] = v;
    }
  }
}

static void launch_dense(const DenseArgs& a, hipStream_t s) {
  VFX_CHECK(a.K % kDK == 0 && a.N % kDN == 0, "k_dense: K = %d, N = %d not multiples of %d, %d", a.K, a.N, kDK, kDN);
  hipLaunchKernelGGL(k_dense, dim3(nblocks_a(a.M, kDM), a.N / kDN), dim3(256), 0, s, a);
  VFX_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// k_gru_seq: one bidirectional GRU layer (hidden 256, PyTorch gate order r, z, n; h_0 = 0)
//   xp (B, T, 1536): per direction d the 768 gate pre-activations W_i{r,z,n} x_t + b_i{r,z,n} (+ b_h{r,z}), at d * 768
//   whhT (2, 256, 768): W_hh of each direction transposed (column k of W_hh = 768 consecutive floats)
//   bhn (2, 256): b_hn, which sits inside r * (W_hn h + b_hn)
//   y (B, T, 512) = [forward | backward]; rows t >= T_b zero.  The backward direction starts at the clip's own last frame T_b - 1.
// ---------------------------------------------------------------------------------------------
constexpr int kGruH = 256, kGruG = 768;
#ifndef VFX_GRU_REGK
#define VFX_GRU_REGK 120
#endif
#ifndef VFX_GRU_BATCH
#define VFX_GRU_BATCH 8
#endif
constexpr int kGruRegK = VFX_GRU_REGK;  // W_hh columns per thread held in VGPRs across the whole sequence
constexpr int kGruLdsK = 48;            // ... in LDS (48 x 768 x 4 B = 144 KiB)
constexpr int kGruStreamK = kGruH - kGruRegK - kGruLdsK;  // ... read from L2 every step
constexpr int kGruBatch = VFX_GRU_BATCH;                  // streamed columns whose loads are in flight together
static_assert(kGruRegK % 4 == 0 && kGruStreamK % kGruBatch == 0 && kGruBatch % 4 == 0, "k_gru_seq column split");

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(768) void k_gru_seq(const float* __restrict__ xp, int T, const int* __restrict__ lens_t,
                                                 const float* whhT, const float* __restrict__ bhn, float* y) {
  __shared__ float wl[kGruLdsK][kGruG];
  __shared__ f32x4 hs4[kGruH / 4];
  __shared__ float gs[kGruG];
  float* const hs = reinterpret_cast<float*>(hs4);
  const int j = threadIdx.x;
  const int b = blockIdx.x, dir = blockIdx.y;
  const int Tb = lens_t ? min(T, lens_t[b]) : T;
  const float* W = whhT + (int64_t)dir * kGruH * kGruG;
  float wr[kGruRegK];
#pragma unroll
  for (int k = 0; k < kGruRegK; ++k) wr[k] = W[(int64_t)k * kGruG + j];
  for (int k = 0; k < kGruLdsK; ++k) wl[k][j] = W[(int64_t)(kGruRegK + k) * kGruG + j];
  const float* Ws = W + (int64_t)(kGruRegK + kGruLdsK) * kGruG + j;
  if (j < kGruH) hs[j] = 0.f;
  float* const yb = y + (int64_t)b * T * 512 + dir * kGruH;
  for (int64_t i = j; i < (int64_t)(T - Tb) * kGruH; i += kGruG) yb[(Tb + i / kGruH) * 512 + i % kGruH] = 0.f;
  const float* const xb = xp + (int64_t)b * T * 1536 + dir * kGruG;
  const float bn = j < kGruH ? bhn[dir * kGruH + j] : 0.f;
  float xr = 0.f, xz = 0.f, xn = 0.f;
  if (j < kGruH && Tb > 0) {
    const float* x0 = xb + (int64_t)(dir ? Tb - 1 : 0) * 1536;
    xr = x0[j];
    xz = x0[kGruH + j];
    xn = x0[2 * kGruH + j];
  }
  __syncthreads();
  for (int s = 0; s < Tb; ++s) {
    const int t = dir ? Tb - 1 - s : s;
    // the next step's input projections, in flight behind this step's product
    float nr = 0.f, nz = 0.f, nn = 0.f;
    if (j < kGruH && s + 1 < Tb) {
      const float* x1 = xb + (int64_t)(dir ? t - 1 : t + 1) * 1536;
      nr = x1[j];
      nz = x1[kGruH + j];
      nn = x1[2 * kGruH + j];
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < kGruRegK / 4; ++k4) {
      const f32x4 h = hs4[k4];
      a0 = fmaf(wr[4 * k4 + 0], h[0], a0);
      a1 = fmaf(wr[4 * k4 + 1], h[1], a1);
      a2 = fmaf(wr[4 * k4 + 2], h[2], a2);
      a3 = fmaf(wr[4 * k4 + 3], h[3], a3);
    }
#pragma unroll 4
    for (int k4 = 0; k4 < kGruLdsK / 4; ++k4) {
      const f32x4 h = hs4[kGruRegK / 4 + k4];
      a0 = fmaf(wl[4 * k4 + 0][j], h[0], a0);
      a1 = fmaf(wl[4 * k4 + 1][j], h[1], a1);
      a2 = fmaf(wl[4 * k4 + 2][j], h[2], a2);
      a3 = fmaf(wl[4 * k4 + 3][j], h[3], a3);
    }
    // the streamed columns: kGruBatch loads in flight at once per round trip to L2 (kGruStreamK / kGruBatch round trips per step)
#pragma unroll 1
    for (int c0 = 0; c0 < kGruStreamK; c0 += kGruBatch) {
      float wv[kGruBatch];
#pragma unroll
      for (int i = 0; i < kGruBatch; ++i) wv[i] = Ws[(int64_t)(c0 + i) * kGruG];
#pragma unroll
      for (int i = 0; i < kGruBatch; i += 4) {
        const f32x4 h = hs4[(kGruRegK + kGruLdsK + c0 + i) / 4];
        a0 = fmaf(wv[i + 0], h[0], a0);
        a1 = fmaf(wv[i + 1], h[1], a1);
        a2 = fmaf(wv[i + 2], h[2], a2);
        a3 = fmaf(wv[i + 3], h[3], a3);
      }
    }
    gs[j] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (j < kGruH) {
      const float r = sigmoid_acc(xr + gs[j]);
      const float z = sigmoid_acc(xz + gs[kGruH + j]);
      const float n = tanhf(fmaf(r, gs[2 * kGruH + j] + bn, xn));
      const float h = fmaf(z, hs[j] - n, n);  // (1 - z) * n + z * h
      hs[j] = h;
      yb[(int64_t)t * 512 + j] = h;
    }
    xr = nr;
    xz = nz;
    xn = nn;
    __syncthreads();
  }
}

static void launch_gru_seq(const float* xp, int B, int T, const int* lens_t, const float* whhT, const float* bhn, float* y,
                           hipStream_t s) {
  VFX_CHECK(B <= 65535, "k_gru_seq: %d clips per launch (at most 65535)", B);
  hipLaunchKernelGGL(k_gru_seq, dim3(B, 2), dim3(kGruG), 0, s, xp, T, lens_t, whhT, bhn, y);
  VFX_HIP(hipGetLastError());
}

// per-clip frame counts of a vfx_analysis_mel call: 64 per launch as kernel arguments (no host copy, capturable)
struct FramesChunk {
  int v[64];
};
__global__ void k_set_frames(int* __restrict__ d, int n, FramesChunk c) {
  if ((int)threadIdx.x < n) d[threadIdx.x] = c.v[threadIdx.x];
}
void launch_set_frames(int* d, const int* host, int B, hipStream_t s) {
  for (int first = 0; first < B; first += 64) {
    FramesChunk c{};
    const int n = std::min(64, B - first);
    for (int i = 0; i < n; ++i) c.v[i] = host[first + i];
    hipLaunchKernelGGL(k_set_frames, dim3(1), dim3(64), 0, s, d + first, n, c);
  }
  VFX_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------------------------
namespace {

struct Staged {
  vfx_handle* h;
  int model;
  std::map<std::string, HostTensor>& m;
  std::set<std::string> used;

  const HostTensor& get(const std::string& name, std::vector<int64_t> shape) {
    auto it = m.find(name);
    VFX_CHECK(it != m.end(), "%s weights: missing tensor '%s'", model == VFX_MODEL_GRU_MEL ? "bi_gru" : "dnn", name.c_str());
    VFX_CHECK(it->second.shape == shape, "%s weights: tensor '%s' has shape %s, expected %s",
              model == VFX_MODEL_GRU_MEL ? "bi_gru" : "dnn", name.c_str(), shape_str(it->second.shape).c_str(),
              shape_str(shape).c_str());
    used.insert(name);
    return it->second;
  }
  static std::string shape_str(const std::vector<int64_t>& s) {
    std::string o = "(";
    for (size_t i = 0; i < s.size(); ++i) o += (i ? ", " : "") + std::to_string(s[i]);
    return o + ")";
  }
  // eval-mode BatchNorm2d(1): gamma * (v - mean) / sqrt(var + 1e-5) + beta  ->  scale * v + shift
  void bn(const std::string& p, float& scale, float& shift) {
    const double g = get(p + ".weight", {1}).data[0], be = get(p + ".bias", {1}).data[0];
    const double mu = get(p + ".running_mean", {1}).data[0], var = get(p + ".running_var", {1}).data[0];
    const double sc = g / std::sqrt(var + 1e-5);
    scale = (float)sc;
    shift = (float)(be - mu * sc);
  }
  DenseW linear(const std::string& p, int K, int N) {
    const HostTensor& w = get(p + ".weight", {N, K});
    const HostTensor& b = get(p + ".bias", {N});
    std::vector<float> wT((size_t)K * N);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) wT[(size_t)k * N + n] = w.data[(size_t)n * K + k];
    DenseW d;
    d.K = K;
    d.N = N;
    d.wT = h->blob.upload(wT);
    d.bias = h->blob.upload(b.data);
    return d;
  }
  // both directions' input projections of one GRU layer as one (K, 1536) Linear; b_hr and b_hz folded into its bias
  DenseW gru_projection(int layer, int K, float** whhT, float** bhn) {
    std::vector<float> wT((size_t)K * 1536), bias(1536), w_hh((size_t)2 * kGruH * kGruG), b_hn(2 * kGruH);
    for (int d = 0; d < 2; ++d) {
      const std::string sfx = "_l" + std::to_string(layer) + (d ? "_reverse" : "");
      const HostTensor& wi = get("2.gru.weight_ih" + sfx, {kGruG, K});
      const HostTensor& wh = get("2.gru.weight_hh" + sfx, {kGruG, kGruH});
      const HostTensor& bi = get("2.gru.bias_ih" + sfx, {kGruG});
      const HostTensor& bh = get("2.gru.bias_hh" + sfx, {kGruG});
      for (int g = 0; g < kGruG; ++g) {
        for (int k = 0; k < K; ++k) wT[(size_t)k * 1536 + d * kGruG + g] = wi.data[(size_t)g * K + k];
        for (int k = 0; k < kGruH; ++k) w_hh[((size_t)d * kGruH + k) * kGruG + g] = wh.data[(size_t)g * kGruH + k];
        bias[d * kGruG + g] = g < 2 * kGruH ? bi.data[g] + bh.data[g] : bi.data[g];
      }
      for (int u = 0; u < kGruH; ++u) b_hn[d * kGruH + u] = bh.data[2 * kGruH + u];
    }
    DenseW p;
    p.K = K;
    p.N = 1536;
    p.wT = h->blob.upload(wT);
    p.bias = h->blob.upload(bias);
    *whhT = h->blob.upload(w_hh);
    *bhn = h->blob.upload(b_hn);
    return p;
  }
};

}  // namespace

std::shared_ptr<AnalysisWeights> build_analysis_weights(vfx_handle* h, int model) {
  VFX_CHECK(h->cfg.n_mels == 128, "analysis modules: n_mels = %d (only 128 is supported)", h->cfg.n_mels);
  auto w = std::make_shared<AnalysisWeights>();
  w->model = model;
  Staged st{h, model, h->staged[model], {}};
  VFX_HIP(hipDeviceSynchronize());
  if (model == VFX_MODEL_GRU_MEL) {
    st.bn("0", w->bn_scale[0], w->bn_shift[0]);
    w->dense.push_back(st.linear("1", 128, 256));
    st.bn("2.bn", w->bn_scale[1], w->bn_shift[1]);
    w->dense.push_back(st.gru_projection(0, 256, &w->whhT[0], &w->bhn[0]));
    w->dense.push_back(st.gru_projection(1, 512, &w->whhT[1], &w->bhn[1]));
    w->dense.push_back(st.linear("4", 512, 256));
    w->dense.push_back(st.linear("6", 256, 128));
  } else {
    VFX_CHECK(model == VFX_MODEL_DNN_MEL, "build_analysis_weights: bad model id %d", model);
    const int width[7] = {128, 256, 512, 1024, 512, 256, 128};
    for (int i = 0; i < 6; ++i) {
      w->dense.push_back(st.linear(std::to_string(i < 5 ? 3 * i : 14), width[i], width[i + 1]));
      if (i < 4) st.bn(std::to_string(3 * i + 2), w->bn_scale[i], w->bn_shift[i]);
    }
  }
  for (auto& kv : st.m)
    VFX_CHECK(st.used.count(kv.first) || (kv.first.size() > 20 && kv.first.compare(kv.first.size() - 20, 20, ".num_batches_tracked") == 0),
              "%s weights: unexpected tensor '%s'", model == VFX_MODEL_GRU_MEL ? "bi_gru" : "dnn", kv.first.c_str());
  return w;
}

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
static BufRef arena_ref(size_t off) {
  BufRef b;
  b.off = off;
  return b;
}

// one Linear: src / dst / mel are BufRefs (caller's tensors or arena slices)
void AnalysisBuilder::dense(const DenseW& d, BufRef src, BufRef dst, int in_log, float in_scale, float in_shift, int in_relu,
                            int out_relu, float out_scale, float out_shift, bool resid, BufRef mel) {
  Plan* pl = pb.plan;
  const int* lens_t = pb.lens_t;
  const int64_t M = (int64_t)B * T;
  const int T_ = T;
  auto res = [pl](const RunCtx& c, const BufRef& b) {
    return b.ext ? c.ext[b.slot] : reinterpret_cast<float*>(pl->bound_base + b.off);
  };
  pl->ops.push_back([=](const RunCtx& c) {
    DenseArgs a{};
    a.x = res(c, src);
    a.wT = d.wT;
    a.bias = d.bias;
    a.resid = resid ? res(c, mel) : nullptr;
    a.y = res(c, dst);
    a.lens_t = lens_t;
    a.flags = c.flags;
    a.M = M;
    a.K = d.K;
    a.N = d.N;
    a.T = T_;
    a.in_log = in_log;
    a.in_relu = in_relu;
    a.out_relu = out_relu;
    a.in_scale = in_scale;
    a.in_shift = in_shift;
    a.out_scale = out_scale;
    a.out_shift = out_shift;
    launch_dense(a, c.stream);
  });
}

void AnalysisBuilder::lin1(BufRef mel, BufRef out) {  // to_log -> BN 0 -> Linear 1 -> BN_GRU.bn
  dense(W.dense[0], mel, out, 1, W.bn_scale[0], W.bn_shift[0], 0, 0, W.bn_scale[1], W.bn_shift[1], false, mel);
}
void AnalysisBuilder::proj(int layer, BufRef src, BufRef xp) {
  dense(W.dense[1 + layer], src, xp, 0, 1.f, 0.f, 0, 0, 1.f, 0.f, false, src);
}
void AnalysisBuilder::gru(int layer, BufRef xp, BufRef out) {
  Plan* pl = pb.plan;
  const int* lens_t = pb.lens_t;
  const float* whhT = W.whhT[layer];
  const float* bhn = W.bhn[layer];
  const int B_ = B, T_ = T;
  auto res = [pl](const RunCtx& c, const BufRef& b) {
    return b.ext ? c.ext[b.slot] : reinterpret_cast<float*>(pl->bound_base + b.off);
  };
  pl->ops.push_back([=](const RunCtx& c) { launch_gru_seq(res(c, xp), B_, T_, lens_t, whhT, bhn, res(c, out), c.stream); });
}
void AnalysisBuilder::lin4(BufRef src, BufRef out) {  // ReLU -> Linear 4 -> ReLU
  dense(W.dense[3], src, out, 0, 1.f, 0.f, 1, 1, 1.f, 0.f, false, src);
}
void AnalysisBuilder::lin6(BufRef src, BufRef mel, BufRef out) {  // Linear 6, + to_log(mel)
  dense(W.dense[4], src, out, 0, 1.f, 0.f, 0, 0, 1.f, 0.f, true, mel);
}
void AnalysisBuilder::fc(int i, BufRef src, BufRef mel, BufRef out) {
  VFX_CHECK(i >= 0 && i < 6, "dnn: no layer %d", i);
  dense(W.dense[i], src, out, i == 0 ? 1 : 0, 1.f, 0.f, 0, i < 5 ? 1 : 0, i < 4 ? W.bn_scale[i] : 1.f, i < 4 ? W.bn_shift[i] : 0.f,
        i == 5, mel);
}

static const AnalysisWeights& analysis_weights(PlanBuilder& pb, int model) {
  VFX_CHECK(model == VFX_MODEL_GRU_MEL || model == VFX_MODEL_DNN_MEL, "model %d is not an analysis module", model);
  const AnalysisWeights* W = pb.h->analysis[model - VFX_MODEL_GRU_MEL].get();
  VFX_CHECK(W, "analysis module %d: weights are not finalized", model);
  return *W;
}

void build_analysis_mel(PlanBuilder& pb, int model, int B, int T, BufRef mel_linear, BufRef logmel_out) {
  AnalysisBuilder ab{pb, analysis_weights(pb, model), B, T};
  const int64_t M = (int64_t)B * T;
  if (model == VFX_MODEL_GRU_MEL) {
    const BufRef a256 = arena_ref(pb.alloc_f(M * 256)), xp = arena_ref(pb.alloc_f(M * 1536)), h1 = arena_ref(pb.alloc_f(M * 512)),
                 h2 = arena_ref(pb.alloc_f(M * 512));
    ab.lin1(mel_linear, a256);
    ab.proj(0, a256, xp);
    ab.gru(0, xp, h1);
    ab.proj(1, h1, xp);
    ab.gru(1, xp, h2);
    ab.lin4(h2, a256);
    ab.lin6(a256, mel_linear, logmel_out);
  } else {
    const BufRef p = arena_ref(pb.alloc_f(M * 1024)), q = arena_ref(pb.alloc_f(M * 1024));
    ab.fc(0, mel_linear, mel_linear, p);
    ab.fc(1, p, mel_linear, q);
    ab.fc(2, q, mel_linear, p);
    ab.fc(3, p, mel_linear, q);
    ab.fc(4, q, mel_linear, p);
    ab.fc(5, p, mel_linear, logmel_out);
  }
}

void build_analysis_piece(PlanBuilder& pb, int model, AnalysisPiece& pc) {
  const std::string name = pc.name ? pc.name : "";
  const int B = pc.B, T = pc.T;
  VFX_CHECK(B > 0 && T > 0, "analysis piece: bad shape");
  AnalysisBuilder ab{pb, analysis_weights(pb, model), B, T};
  const int64_t M = (int64_t)B * T;
  pc.nin = 0;
  auto input = [&](int c) {
    const BufRef b = arena_ref(pb.alloc_f(M * c));
    pc.in_off[pc.nin] = b.off;
    pc.in_n[pc.nin++] = M * c;
    return b;
  };
  auto output = [&](int c) {
    const BufRef b = arena_ref(pb.alloc_f(M * c));
    pc.out_off = b.off;
    pc.out_n = M * c;
    return b;
  };
  if (model == VFX_MODEL_GRU_MEL) {
    if (name == "lin1") {
      const BufRef mel = input(128);
      ab.lin1(mel, output(256));
    } else if (name == "proj0" || name == "proj1") {
      const int layer = name[4] - '0';
      const BufRef src = input(layer ? 512 : 256);
      ab.proj(layer, src, output(1536));
    } else if (name == "gru0" || name == "gru1") {
      const BufRef xp = input(1536);
      ab.gru(name[3] - '0', xp, output(512));
    } else if (name == "lin4") {
      const BufRef src = input(512);
      ab.lin4(src, output(256));
    } else if (name == "lin6") {
      const BufRef src = input(256), mel = input(128);
      ab.lin6(src, mel, output(128));
    } else {
      VFX_CHECK(false, "analysis piece: bi_gru has no piece '%s'", name.c_str());
    }
  } else {
    const int width[7] = {128, 256, 512, 1024, 512, 256, 128};
    VFX_CHECK(name.size() == 3 && name.compare(0, 2, "fc") == 0 && name[2] >= '0' && name[2] <= '5',
              "analysis piece: dnn has no piece '%s'", name.c_str());
    const int i = name[2] - '0';
    const BufRef src = input(width[i]);
    const BufRef mel = i == 5 ? input(128) : src;
    ab.fc(i, src, mel, output(width[i + 1]));
  }
}

}  // namespace vfx
