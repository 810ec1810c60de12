// front_end.cpp -- the tables of the STFT / mel front end (stft.hip): window, twiddles, mel filterbank, vocoder band weights.
#include <cmath>

#include "vfx_internal.h"

namespace vfx {

// ---------------------------------------------------------------------------------------------
// front-end tables
// ---------------------------------------------------------------------------------------------
static double hz_to_mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }

// (NB, NM) filterbank -> its non-zeros band-major (val), the first bin of every band (start) and the bands' offsets into val (off)
static void pack_filterbank(const float* fb, int NB, int NM, std::vector<float>& val, std::vector<int>& start, std::vector<int>& off) {
  val.clear();
  start.assign(NM, 0);
  off.assign(NM + 1, 0);
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
}

void set_mel_filterbank(vfx_handle* h, const float* fb) {
  std::vector<float> val;
  std::vector<int> start, off;
  pack_filterbank(fb, h->cfg.n_fft / 2 + 1, h->cfg.n_mels, val, start, off);
  h->fe.fb_val = h->blob.upload(val);
  h->fe.fb_nnz = (int)val.size();
  h->fe.fb_start = h->blob.upload_i(start);
  h->fe.fb_off = h->blob.upload_i(off);
}

// ---------------------------------------------------------------------------------------------
// the 743-point front end of the scores at 16 kHz (stft_dft.hip)
// ---------------------------------------------------------------------------------------------
static void upload_score16k_filterbank(vfx_handle* h) {
  std::vector<float> fb = h->fe16.fb_host;
  if (fb.empty()) {  // MelScale(n_mels=80, sample_rate=16000, n_stft=372), HTK, in float64 (the Python shim hands over the reference's
                     // float32 evaluation: "mel16k.fb")
    const double fmax = kDftRate / 2;
    std::vector<double> fpts(kDftMels + 2);
    for (int i = 0; i < kDftMels + 2; ++i) fpts[i] = 700.0 * (std::pow(10.0, hz_to_mel(fmax) * i / (kDftMels + 1) / 2595.0) - 1.0);
    fb.resize((size_t)kDftBins * kDftMels);
    for (int f = 0; f < kDftBins; ++f) {
      const double hz = fmax * f / (kDftBins - 1);
      for (int m = 0; m < kDftMels; ++m) {
        const double up = (hz - fpts[m]) / (fpts[m + 1] - fpts[m]);
        const double down = (fpts[m + 2] - hz) / (fpts[m + 2] - fpts[m + 1]);
        fb[(size_t)f * kDftMels + m] = (float)std::max(0.0, std::min(up, down));
      }
    }
  }
  std::vector<float> val;
  std::vector<int> start, off;
  pack_filterbank(fb.data(), kDftBins, kDftMels, val, start, off);
  h->fe16.fb_val = h->blob.upload(val);
  h->fe16.fb_start = h->blob.upload_i(start);
  h->fe16.fb_off = h->blob.upload_i(off);
}

const Score16kTables& ensure_score16k_tables(vfx_handle* h) {
  if (h->fe16.table) return h->fe16;
  // tab[n][k] = w[n] cos(a), tab[n][kDftCols + k] = -w[n] sin(a), a = 2 pi (k n mod 743) / 743: the angle index reduced as an integer,
  // the product formed in float64 and rounded to float32 once.  Row 743 and the columns from 372 up are zeros.
  // Stored in the order the kernel's B fragments are read (dft_table_index): the eight values a lane needs for a pass of 8 values
  // of n side by side.
  std::vector<float> tab((size_t)kDftK * 2 * kDftCols, 0.f);
  for (int n = 0; n < kDftN; ++n) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * n / kDftN);
    for (int k = 0; k < kDftBins; ++k) {
      const double a = 2.0 * M_PI * (double)((k * n) % kDftN) / kDftN;
      tab[dft_table_index(n, k, 0)] = (float)(w * std::cos(a));
      tab[dft_table_index(n, k, 1)] = (float)(-(w * std::sin(a)));
    }
  }
  upload_score16k_filterbank(h);
  h->fe16.table = h->blob.upload(tab);
  return h->fe16;
}

void set_score16k_filterbank(vfx_handle* h, const float* fb) {
  h->fe16.fb_host.assign(fb, fb + (size_t)kDftBins * kDftMels);
  if (h->fe16.table) upload_score16k_filterbank(h);  // (the caller has synchronised the device)
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
