// front_end.cpp -- the tables of the STFT / mel front end (stft.hip): window, twiddles, mel filterbank, vocoder band weights.
#include <cmath>

#include "vfx_internal.h"

namespace vfx {

// ---------------------------------------------------------------------------------------------
// front-end tables
// ---------------------------------------------------------------------------------------------
static double hz_to_mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }

void set_mel_filterbank(vfx_handle* h, const float* fb) {
  const int NB = h->cfg.n_fft / 2 + 1, NM = h->cfg.n_mels;
  std::vector<float> val;
  std::vector<int> start(NM), off(NM + 1);
  for (int m = 0; m < NM; ++m) {
    int lo = -1, hi = -1;
    for (int f = 0; f < NB; ++f)
      if (fb[(size_t)f * NM + m] != 0.f) {
        if (lo < 0) lo = f;
        hi = f;
      }
    off[m] = (int)val.size();
    start[m] = lo < 0 ? 0 : lo;
    if (lo >= 0)
      for (int f = lo; f <= hi; ++f) val.push_back(fb[(size_t)f * NM + m]);
  }
  off[NM] = (int)val.size();
  h->fe.fb_val = h->blob.upload(val);
  h->fe.fb_nnz = (int)val.size();
  h->fe.fb_start = h->blob.upload_i(start);
  h->fe.fb_off = h->blob.upload_i(off);
}

void init_front_end(vfx_handle* h) {
  const int N = h->cfg.n_fft;
  VFX_CHECK(N == 2048, "only n_fft = 2048 is supported (got %d)", N);
  VFX_CHECK(h->cfg.n_mels == 128, "only n_mels = 128 is supported (got %d)", h->cfg.n_mels);
  std::vector<float> win(N), tw(2 * (N / 2)), rtw(2 * (N / 2 + 1));
  for (int n = 0; n < N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / N));
  for (int m = 0; m < N / 2; ++m) {
    tw[2 * m] = (float)std::cos(2.0 * M_PI * m / (N / 2));
    tw[2 * m + 1] = (float)(-std::sin(2.0 * M_PI * m / (N / 2)));
  }
  for (int k = 0; k <= N / 2; ++k) {
    rtw[2 * k] = (float)std::cos(2.0 * M_PI * k / N);
    rtw[2 * k + 1] = (float)(-std::sin(2.0 * M_PI * k / N));
  }
  h->fe.window = h->blob.upload(win);
  h->fe.twiddle = h->blob.upload(tw);
  h->fe.rtwiddle = h->blob.upload(rtw);

  // Default HTK mel filterbank (mel_scale.py:131-221) evaluated in double precision.  The
  // reference evaluates it with float32 torch ops; the Python shim therefore overrides this
  // table with the bit-identical one via vfx_load_tensor(VFX_MODEL_FRONTEND, "mel.fb").
  const int NB = N / 2 + 1, NM = h->cfg.n_mels;
  const double fmax = (double)(h->cfg.sample_rate / 2);
  std::vector<double> fpts(NM + 2);
  for (int i = 0; i < NM + 2; ++i) {
    const double m = hz_to_mel(0.0) + (hz_to_mel(fmax) - hz_to_mel(0.0)) * i / (NM + 1);
    fpts[i] = 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
  }
  std::vector<float> fb((size_t)NB * NM);
  for (int f = 0; f < NB; ++f) {
    const double hz = fmax * f / (NB - 1);
    for (int m = 0; m < NM; ++m) {
      const double up = (hz - fpts[m]) / (fpts[m + 1] - fpts[m]);
      const double down = (fpts[m + 2] - hz) / (fpts[m + 2] - fpts[m + 1]);
      fb[(size_t)f * NM + m] = (float)std::max(0.0, std::min(up, down));
    }
  }
  set_mel_filterbank(h, fb.data());

  // vocoder band weights: get_mel_weig (pytorch_util.py:141-155), base 10
  std::vector<float> invw(NM);
  const double norm0 = (fpts[2] - fpts[0]) / 2.0;
  for (int m = 0; m < NM; ++m) invw[m] = (float)(1.0 / (((fpts[m + 2] - fpts[m]) / 2.0) / norm0));
  h->fe.voc_inv_weight = h->blob.upload(invw);
}

}  // namespace vfx
