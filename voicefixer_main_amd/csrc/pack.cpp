// pack.cpp -- convolution weights in MFMA fragment order (conv.hip reads them with one 16-byte load per lane).
#include <cmath>
#include <cstring>

#include "vfx_internal.h"

namespace vfx {

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
// PyTorch Conv weight (Cout, CinTotal, KH, KW) -> [C/32][ntaps][Cout][32] for input channels
// [c_lo, c_lo + C); taps are (kh, kw) pairs.
static inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// Rows -> MFMA fragment order.  Input: consecutive (chunk, tap) blocks of [Cout][32] floats.
// Output per block: [Cout/32][1024 floats]; inside a 1024-float cout block
//   split-bf16: 4 fragments (s, hl) = (k 0..15 | 16..31) x (hi | lo), each [64 lanes][8 bf16]:
//               lane l holds W[cout = 32*nb + (l & 31)][k = 16*s + 8*(l >> 5) + 0..7], w = hi + lo up
//               to 2^-17 relative;
//   fp32:       4 fragments g (k8 groups), each [64 lanes][4 floats]:
//               lane l holds W[cout = 32*nb + (l & 31)][k = 8*g + 4*(l >> 5) + 0..3].
// A wave reads one fragment with ONE coalesced 16-byte-per-lane load (conv.hip).
static inline uint16_t f16_rne(float f) {
  const float c = std::min(std::max(f, -65504.f), 65504.f);
  const _Float16 h = (_Float16)c;
  uint16_t u;
  memcpy(&u, &h, sizeof(u));
  return u;
}

// mode: 0 = fp32 fragments, 1 = split-bf16 (hi, lo), 2 = fp16 in the hi fragments (lo fragments zero: never loaded),
//       3 = fp16, 64-channel chunks (conv_chunk(mode) input channels per block): the four fragments of a cout block are
//           the K = 16 steps k 0..15 | 16..31 | 32..47 | 48..63, lane l holds W[cout = 32*nb + (l & 31)][k = 16*f + 8*(l >> 5) + 0..7]
//           -- the weights of a convolution whose source is an activated fp16 tensor (k_conv, H64)
int conv_chunk(int mode) { return mode == 3 ? 64 : kKC; }

bool& f16_weight_issue() {
  static thread_local bool issue = false;
  return issue;
}

void rows_to_fragments(std::vector<float>& packed, int Cout, int mode) {
  const bool split = mode != 0;
  if (mode == 2 || mode == 3) {
    // fp16 operands: f16_rne clamps and flushes silently, and no device flag sees a WEIGHT.  A tensor whose largest weight
    // is outside the fp16 range, or so deep in fp16's subnormal range (< 2^-17: fewer than 8 significant bits for the
    // LARGEST weight, less for the others) that the products lose the mode's accuracy, marks the weight set as "needs
    // strict arithmetic" (f16_weight_issue(); vocoder.cpp): every call on it raises VFX_FLAG_F16_SATURATED, so the
    // model-level calls re-run on split-bf16 operands and a raw caller sees the flag.  Measured
    // (tests/test_gpu_models.py): a tensor at 3e-5 (9 bits) still holds 55 dB, one at 3e-7 gives 18 dB.
    float wmax = 0.f;
    bool finite = true;
    for (float v : packed) {
      finite = finite && std::isfinite(v);
      wmax = std::max(wmax, std::fabs(v));
    }
    VFX_CHECK(finite, "precision 2: a convolution weight is not finite");
    if (wmax > 65504.f || (wmax != 0.f && wmax < 6.103515625e-05f / 8.f)) f16_weight_issue() = true;
  }
  const int kc = conv_chunk(mode);
  const size_t blk = (size_t)Cout * kc;         // input floats per (chunk, tap) block
  const size_t oblk = (size_t)Cout * kKC;       // output floats per block: Cout / 32 cout blocks of 1024 floats
  std::vector<float> res(packed.size() / blk * oblk);
  size_t oo = 0;
  for (size_t o = 0; o + blk <= packed.size(); o += blk, oo += oblk) {
    const float* in = &packed[o];
    for (int nb = 0; nb < Cout / 32; ++nb) {
      float* out = &res[oo + (size_t)nb * 1024];
      for (int f = 0; f < 4; ++f)
        for (int l = 0; l < 64; ++l) {
          const float* row = in + (size_t)(nb * 32 + (l & 31)) * kc;
          float* dst = out + (f * 64 + l) * 4;
          if (mode == 3) {
            uint16_t q[8];
            for (int j = 0; j < 8; ++j) q[j] = f16_rne(row[16 * f + 8 * (l >> 5) + j]);
            memcpy(dst, q, sizeof(q));
          } else if (split) {
            const int s2 = f >> 1, lo = f & 1;
            uint16_t q[8];
            for (int j = 0; j < 8; ++j) {
              const float v = row[16 * s2 + 8 * (l >> 5) + j];
              if (mode == 2) {
                q[j] = lo ? (uint16_t)0 : f16_rne(v);
              } else {
                const uint16_t hi = bf16_rne(v);
                q[j] = lo ? bf16_rne(v - bf16_to_f32(hi)) : hi;
              }
            }
            memcpy(dst, q, sizeof(q));
          } else {
            for (int e = 0; e < 4; ++e) dst[e] = row[8 * f + 4 * (l >> 5) + e];
          }
        }
    }
  }
  packed.swap(res);
}

std::vector<float> pack_conv(const float* w, int Cout, int CinTotal, int KH, int KW, int c_lo, int C,
                             const std::vector<std::pair<int, int>>& taps, int mode) {
  const int nt = (int)taps.size(), kc = conv_chunk(mode);
  VFX_CHECK(C % kc == 0, "pack_conv: %d input channels do not split into %d-channel chunks", C, kc);
  std::vector<float> out((size_t)C * nt * Cout);
  for (int ch = 0; ch < C / kc; ++ch)
    for (int t = 0; t < nt; ++t)
      for (int n = 0; n < Cout; ++n)
        for (int cc = 0; cc < kc; ++cc) {
          const int c = c_lo + ch * kc + cc;
          out[(((size_t)ch * nt + t) * Cout + n) * kc + cc] =
              w[(((size_t)n * CinTotal + c) * KH + taps[t].first) * KW + taps[t].second];
        }
  rows_to_fragments(out, Cout, mode);
  return out;
}

// PyTorch ConvTranspose weight (Cin, Cout, KH, KW) -> [Cin/chunk][ntaps][Cout][chunk] -> fragment order.
std::vector<float> pack_conv_transposed(const float* w, int Cin, int Cout, int KH, int KW,
                                        const std::vector<std::pair<int, int>>& taps, int mode) {
  const int nt = (int)taps.size(), kc = conv_chunk(mode);
  VFX_CHECK(Cin % kc == 0, "pack_conv_transposed: %d input channels do not split into %d-channel chunks", Cin, kc);
  std::vector<float> out((size_t)Cin * nt * Cout);
  for (int ch = 0; ch < Cin / kc; ++ch)
    for (int t = 0; t < nt; ++t)
      for (int n = 0; n < Cout; ++n)
        for (int cc = 0; cc < kc; ++cc) {
          const int c = ch * kc + cc;
          out[(((size_t)ch * nt + t) * Cout + n) * kc + cc] =
              w[(((size_t)c * Cout + n) * KH + taps[t].first) * KW + taps[t].second];
        }
  rows_to_fragments(out, Cout, mode);
  return out;
}

}  // namespace vfx
