// api.cpp -- error text, the stream turns and the extern "C" entry points of libvfx.so.
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <numeric>

#include "clip_batch.h"
#include "stream.h"
#include "vfx_internal.h"

namespace vfx {

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

bool stream_turns_enabled() {
  static const bool on = [] {
    const char* e = getenv("VFX_NO_STREAM_TURNS");
    return !(e && atoi(e) != 0);
  }();
  return on;
}

DeviceTurn& device_turn(int device) {
  static DeviceTurn turns[64];
  return turns[(unsigned)device % 64u];
}

}  // namespace vfx

// =============================================================================================
// extern "C"
// =============================================================================================
using namespace vfx;

// body(first clip, clips) over B clips, `step` at a time; stops at the first non-zero return code
template <class Body>
static int for_sub_batches(int B, int step, Body body) {
  for (int b = 0; b < B; b += step) {
    const int rc = body(b, std::min(step, B - b));
    if (rc) return rc;
  }
  return 0;
}

extern "C" {

const char* vfx_last_error(void) { return vfx::g_err.c_str(); }

int vfx_default_config(vfx_config* cfg) {
  if (!cfg) return 1;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->sample_rate = 44100;
  cfg->n_fft = 2048;
  cfg->hop = 441;
  cfg->n_mels = 128;
  cfg->voc_cond_channels = 512;
  cfg->voc_cond_layers = 5;
  cfg->voc_channels = 1024;
  cfg->voc_n_stages = 4;
  const int scales[4] = {7, 7, 3, 3};
  for (int i = 0; i < 4; ++i) {
    cfg->voc_scales[i] = scales[i];
    cfg->voc_depth[i] = 8;
  }
  cfg->voc_dilation_base = 3;
  cfg->voc_min_db = -115.f;
  cfg->voc_amp_floor = 1e-5f;
  cfg->voc_norm_range = 4.f;
  cfg->voc_up_slope = 0.2f;
  cfg->voc_res_slope = 0.01f;
  cfg->precision = 1;
  return 0;
}

int vfx_create(int device, const vfx_config* cfg, vfx_handle** out) {
  VFX_API_BEGIN
  VFX_CHECK(out != nullptr, "vfx_create: out is NULL");
  DeviceGuard device_guard_(device);  // the caller's current device is left as it was
  auto h = std::make_unique<vfx_handle>();
  h->device = device;
  if (cfg) h->cfg = *cfg; else vfx_default_config(&h->cfg);
  VFX_CHECK(h->cfg.voc_n_stages >= 1 && h->cfg.voc_n_stages <= VFX_MAX_STAGES, "bad voc_n_stages");
  VFX_CHECK((h->cfg.tuning & ~4095) == 0, "vfx_create: unknown bits in vfx_config.tuning (0x%x)", h->cfg.tuning);
  if (h->cfg.tuning) {  // never silent: a non-default kernel selection is announced
    static const char* names[] = {"NO_FUSED_STACKS", "NO_FUSED_WIDE", "NO_FUSED_UNET", "NO_PERSISTENT_C64", "NO_PAIRS", "NO_SPLITK",
                                  "F32_TRUNK", "SMALL_2D_TILES", "DEBUG_POISON_ARENA", "NO_FUSED_UPSAMPLERS", "OLD_BLOCK2D", "TWO_LAUNCH_UPSAMPLERS"};
    std::string msg;
    for (int b = 0; b < 12; ++b)
      if (h->cfg.tuning & (1 << b)) msg += std::string(msg.empty() ? "" : " | ") + "VFX_TUNE_" + names[b];
    fprintf(stderr, "[libvfx] handle on device %d uses non-default kernel selection: tuning = 0x%x (%s)\n", device, h->cfg.tuning,
            msg.c_str());
  }
  init_front_end(h.get());
  {
    std::vector<float> ones(kIdentityLen, 1.f), zeros(kIdentityLen, 0.f);
    h->d_ones = h->blob.upload(ones);
    h->d_zeros = h->blob.upload(zeros);
  }
  h->d_flags = static_cast<int*>(h->blob.alloc(sizeof(int)));
  VFX_HIP(hipMemset(h->d_flags, 0, sizeof(int)));
  h->d_lens = static_cast<int*>(h->blob.alloc(kLensRows * kMaxVarlenClips * sizeof(int)));
  VFX_HIP(hipMemset(h->d_lens, 0, kLensRows * kMaxVarlenClips * sizeof(int)));
  *out = h.release();
  VFX_API_END
}

int vfx_destroy(vfx_handle* h) {
  if (!h) return 0;
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  h->plans.clear();
  h->retired.clear();
  delete h;  // (frees the arena and the other grow-only buffers)
  if (prev >= 0) (void)hipSetDevice(prev);
  return 0;
}

int vfx_load_tensor(vfx_handle* h, int model, const char* name, const float* data, const int64_t* shape, int ndim) {
  VFX_API_BEGIN
  VFX_CHECK(h && name && data, "vfx_load_tensor: NULL argument");
  VFX_CHECK(model >= 0 && model <= VFX_MODEL_DNN_MEL, "vfx_load_tensor: bad model id %d", model);
  HostTensor t;
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    t.shape.push_back(shape[i]);
    n *= shape[i];
  }
  t.data.assign(data, data + n);
  h->staged[model][name] = std::move(t);
  VFX_API_END
}

int vfx_finalize_weights(vfx_handle* h, int model) {
  VFX_API_BEGIN_H(h)
  // (no plan reads the scoring tables at 16 kHz: loading them alone leaves the plans, pinned ones included, as they are)
  const bool score16k_only = model == VFX_MODEL_FRONTEND && h->staged[model].size() == 1 && h->staged[model].count("mel16k.fb");
  if (!score16k_only) h->plans.clear();
  if (model == VFX_MODEL_UNET_MEL || model == VFX_MODEL_UNET_SPEC) {
    h->unet[model] = build_unet_weights(h, model);
  } else if (model == VFX_MODEL_VOCODER) {
    h->voc = build_vocoder_weights(h);
  } else if (model == VFX_MODEL_GRU_MEL || model == VFX_MODEL_DNN_MEL) {
    h->analysis[model - VFX_MODEL_GRU_MEL] = nullptr;
    h->analysis[model - VFX_MODEL_GRU_MEL] = build_analysis_weights(h, model);
  } else if (model == VFX_MODEL_FRONTEND) {
    auto it = h->staged[model].find("mel.fb");
    if (it != h->staged[model].end()) {
      VFX_CHECK(it->second.shape.size() == 2 && it->second.shape[0] == h->cfg.n_fft / 2 + 1 &&
                    it->second.shape[1] == h->cfg.n_mels,
                "mel.fb must be (%d, %d)", h->cfg.n_fft / 2 + 1, h->cfg.n_mels);
      VFX_HIP(hipDeviceSynchronize());
      set_mel_filterbank(h, it->second.data.data());
    }
    it = h->staged[model].find("mel16k.fb");
    if (it != h->staged[model].end()) {
      VFX_CHECK(it->second.shape.size() == 2 && it->second.shape[0] == kDftBins && it->second.shape[1] == kDftMels,
                "mel16k.fb must be (%d, %d)", kDftBins, kDftMels);
      VFX_HIP(hipDeviceSynchronize());
      set_score16k_filterbank(h, it->second.data.data());
    }
  } else {
    VFX_CHECK(false, "vfx_finalize_weights: bad model id %d", model);
  }
  h->staged[model].clear();
  VFX_API_END
}

int vfx_unpin_plans(vfx_handle* h) {
  VFX_API_BEGIN_H(h)
  for (auto& kv : h->plans) kv.second->pinned = false;
  VFX_API_END
}

// Read-and-clear only the bits in `mask`: the other sticky bits stay raised for whoever checks them later (a deferred
// saturation check of the vocoder must survive the UNet stage's negative-input check, models.VoiceFixer.forward).
int vfx_take_flags_masked(vfx_handle* h, void* stream, int mask, int* flags_out) {
  VFX_API_BEGIN_H(h)
  VFX_CHECK(flags_out, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int v = 0;
  VFX_HIP(hipMemcpyAsync(&v, h->d_flags, sizeof(int), hipMemcpyDeviceToHost, s));
  VFX_HIP(hipMemsetAsync(h->d_flags, 0, sizeof(int), s));
  VFX_HIP(hipStreamSynchronize(s));
  if (v & ~mask) launch_or_flags(h->d_flags, v & ~mask, s);  // in stream order, before anything the caller enqueues next
  *flags_out = v & mask;
  VFX_API_END
}

// every bit: nothing is left to raise again
int vfx_take_flags(vfx_handle* h, void* stream, int* flags_out) { return vfx_take_flags_masked(h, stream, ~0, flags_out); }

// The two halves of a turn for work this library does not enqueue itself: the replay of a hipGraph captured from its calls
// (a captured call is exempt from the turns, so its replay would otherwise overlap a live call of another stream).
int vfx_turn_begin(int device, void* stream) {
  VFX_API_BEGIN
  DeviceGuard device_guard_(device);
  if (stream_turns_enabled()) {
    DeviceTurn& d = device_turn(device);
    std::lock_guard<std::mutex> lock(d.mu);
    turn_wait(d, static_cast<hipStream_t>(stream));
  }
  VFX_API_END
}

int vfx_turn_end(int device, void* stream) {
  VFX_API_BEGIN
  DeviceGuard device_guard_(device);
  if (stream_turns_enabled()) {
    DeviceTurn& d = device_turn(device);
    std::lock_guard<std::mutex> lock(d.mu);
    VFX_CHECK(turn_record(d, static_cast<hipStream_t>(stream)), "vfx_turn_end: cannot record the end of the turn on this stream");
  }
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// front-end
// ---------------------------------------------------------------------------------------------
static int frames_of(const vfx_handle* h, int L) { return L / h->cfg.hop + 1; }

int vfx_stft_mel(vfx_handle* h, const float* wav, int B, int L, float* mel, float* sp, float* cosp, float* sinp,
                 int log10_mel, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(wav, "NULL argument");
  VFX_CHECK(B > 0 && L > h->cfg.n_fft / 2, "vfx_stft_mel: need B > 0 and L > n_fft/2 (reflect padding), got B=%d L=%d", B, L);
  launch_stft_mel(h->fe, wav, B, L, frames_of(h, L), mel, sp, cosp, sinp, log10_mel, h->cfg.hop, 1e-8f,
                  static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_stft_phase(vfx_handle* h, const float* wav, int B, int L, float* sp, float* cosp, float* sinp, float eps,
                   void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(wav && (sp || cosp || sinp), "NULL argument");
  VFX_CHECK(B > 0 && L > h->cfg.n_fft / 2, "vfx_stft_phase: need B > 0 and L > n_fft/2 (reflect padding), got B=%d L=%d", B, L);
  VFX_CHECK(eps >= 0.f, "vfx_stft_phase: eps must be >= 0 (got %g)", (double)eps);
  launch_stft_mel(h->fe, wav, B, L, frames_of(h, L), nullptr, sp, cosp, sinp, 0, h->cfg.hop, eps,
                  static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_stft_lowpass(vfx_handle* h, const float* wav, int B, int L, const int* lengths, const int* cut_bins, float* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(wav && lengths && cut_bins && out && B > 0 && L > 0, "vfx_stft_lowpass: bad argument");
  VFX_CHECK(h->cfg.n_fft == 2048, "vfx_stft_lowpass: needs the 44.1 kHz front end (n_fft 2048)");
  for (int b = 0; b < B; ++b) {
    VFX_CHECK(lengths[b] > h->cfg.n_fft / 2 && lengths[b] <= L,
              "vfx_stft_lowpass: clip %d has %d samples (need n_fft/2 = %d < length <= L = %d: reflect padding)", b, lengths[b],
              h->cfg.n_fft / 2, L);
    VFX_CHECK(cut_bins[b] >= 0, "vfx_stft_lowpass: clip %d has cut-off bin %d (need >= 0)", b, cut_bins[b]);
  }
  // (compared as integers: the two ranges of B * L floats)
  const uintptr_t w0 = reinterpret_cast<uintptr_t>(wav), o0 = reinterpret_cast<uintptr_t>(out);
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)L * sizeof(float);
  VFX_CHECK(o0 + bytes <= w0 || w0 + bytes <= o0, "vfx_stft_lowpass: out overlaps wav (a workgroup reads samples its neighbours write)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_l = h->lens_row(LENS_LOWPASS_SAMPLES);
  int* const d_c = h->lens_row(LENS_LOWPASS_CUT);
  for (int b0 = 0; b0 < B; b0 += kMaxVarlenClips) {  // (a clip's samples do not depend on the launch it is in)
    const int n = std::min(kMaxVarlenClips, B - b0);
    launch_set_frames(d_l, lengths + b0, n, s);
    launch_set_frames(d_c, cut_bins + b0, n, s);
    launch_stft_lowpass(h->fe, wav + (int64_t)b0 * L, n, L, h->cfg.hop, d_l, d_c, out + (int64_t)b0 * L, s);
  }
  VFX_API_END
}

// [p, p + bytes) and [q, q + bytes) share no byte (compared as integers)
static bool ranges_disjoint(const void* p, const void* q, uintptr_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a + bytes <= b || b + bytes <= a;
}

int vfx_stft_splice(vfx_handle* h, const float* x, const float* y, int B, int L, const int* lengths, const int* cut_bins, int ramp,
                    const float* gains, float* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && y && lengths && cut_bins && out, "vfx_stft_splice: NULL argument");
  VFX_CHECK(B > 0 && L > 0, "vfx_stft_splice: need B > 0 and L > 0, got B=%d L=%d", B, L);
  VFX_CHECK(h->cfg.n_fft == 2048, "vfx_stft_splice: needs the 44.1 kHz front end (n_fft 2048)");
  VFX_CHECK(ramp >= 0, "vfx_stft_splice: ramp = %d bins (need >= 0)", ramp);
  std::vector<int> gbits(B);  // the gains as float32 bit patterns: they travel in an int row of d_lens
  for (int b = 0; b < B; ++b) {
    VFX_CHECK(lengths[b] > h->cfg.n_fft / 2 && lengths[b] <= L,
              "vfx_stft_splice: clip %d has %d samples (need n_fft/2 = %d < length <= L = %d: reflect padding)", b, lengths[b],
              h->cfg.n_fft / 2, L);
    VFX_CHECK(cut_bins[b] >= 0, "vfx_stft_splice: clip %d has cut-off bin %d (need >= 0)", b, cut_bins[b]);
    const float g = gains ? gains[b] : 1.f;
    VFX_CHECK(std::isfinite(g), "vfx_stft_splice: clip %d has gain %g (need a finite gain)", b, (double)g);
    std::memcpy(&gbits[b], &g, sizeof(float));
  }
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)L * sizeof(float);
  VFX_CHECK(ranges_disjoint(out, x, bytes), "vfx_stft_splice: out overlaps x (a workgroup reads samples its neighbours write)");
  VFX_CHECK(ranges_disjoint(out, y, bytes), "vfx_stft_splice: out overlaps y (a workgroup reads samples its neighbours write)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_l = h->lens_row(LENS_SPLICE_SAMPLES);
  int* const d_c = h->lens_row(LENS_SPLICE_CUT);
  int* const d_g = h->lens_row(LENS_SPLICE_GAIN);
  for (int b0 = 0; b0 < B; b0 += kSpliceMaxClips) {  // (a clip's samples do not depend on the launch it is in)
    const int n = std::min(kSpliceMaxClips, B - b0);
    launch_set_frames(d_l, lengths + b0, n, s);
    launch_set_frames(d_c, cut_bins + b0, n, s);
    launch_set_frames(d_g, gbits.data() + b0, n, s);
    launch_stft_splice(h->fe, x + (int64_t)b0 * L, y + (int64_t)b0 * L, n, L, h->cfg.hop, d_l, d_c, d_g, ramp, out + (int64_t)b0 * L, s);
  }
  VFX_API_END
}

int vfx_band_power(vfx_handle* h, const float* a, const float* b, int B, int Lmax, const int* lengths, const int* lo_bins,
                   const int* hi_bins, double* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(a && b && lo_bins && hi_bins && out, "vfx_band_power: NULL argument");
  VFX_CHECK(B > 0 && Lmax > 0, "vfx_band_power: need B > 0 and Lmax > 0, got B=%d Lmax=%d", B, Lmax);
  VFX_CHECK(h->cfg.n_fft == 2048, "vfx_band_power: needs the 44.1 kHz front end (n_fft 2048)");
  const int hop = h->cfg.hop, half = h->cfg.n_fft / 2, nbins = half + 1;
  std::vector<int> host(2 * (size_t)B);  // samples | frames
  for (int i = 0; i < B; ++i) {
    const int Lb = lengths ? lengths[i] : Lmax;
    VFX_CHECK(Lb > half && Lb <= Lmax, "vfx_band_power: clip %d has %d samples (need %d < length <= Lmax = %d: reflect padding)", i, Lb, half,
              Lmax);
    VFX_CHECK(lo_bins[i] >= 0 && hi_bins[i] <= nbins && hi_bins[i] >= lo_bins[i],
              "vfx_band_power: clip %d has the band [%d, %d) (need 0 <= lo <= hi <= %d)", i, lo_bins[i], hi_bins[i], nbins);
    host[i] = Lb;
    host[(size_t)B + i] = Lb / hop + 1;
  }
  const uintptr_t in_bytes = (uintptr_t)B * (uintptr_t)Lmax * sizeof(float), out_bytes = (uintptr_t)B * 2 * sizeof(double);
  for (const float* in : {a, b}) {
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
    VFX_CHECK(o0 + out_bytes <= i0 || i0 + in_bytes <= o0, "vfx_band_power: out overlaps %s", in == a ? "a" : "b");
  }
  const int T = frames_of(h, Lmax);
  const int step = std::min(B, kSpliceMaxClips);
  double* const ws = reinterpret_cast<double*>(h->scratch.ensure(
      h, (size_t)step * T * 2 * sizeof(double), 8, "the varlen scratch would have to grow from %zu to %zu bytes, but a hipGraph was captured "
      "from plan '%s': run the largest vfx_band_power batch once BEFORE capturing"));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_n = h->lens_row(LENS_POWER_SAMPLES);
  int* const d_f = h->lens_row(LENS_POWER_FRAMES);
  int* const d_lo = h->lens_row(LENS_POWER_LO);
  int* const d_hi = h->lens_row(LENS_POWER_HI);
  for (int b0 = 0; b0 < B; b0 += step) {  // (a clip's numbers do not depend on the launch it is in)
    const int n = std::min(step, B - b0);
    launch_set_frames(d_n, host.data() + b0, n, s);
    launch_set_frames(d_f, host.data() + B + b0, n, s);
    launch_set_frames(d_lo, lo_bins + b0, n, s);
    launch_set_frames(d_hi, hi_bins + b0, n, s);
    launch_pair_band_power(h->fe, a + (int64_t)b0 * Lmax, b + (int64_t)b0 * Lmax, n, Lmax, T, d_n, d_lo, d_hi, d_f, hop, 1e-8f, ws,
                           out + (int64_t)b0 * 2, s);
  }
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// bandwidth detector (tools/utils.py:33-44 load_wav_energy on the device: band.hip)
// ---------------------------------------------------------------------------------------------
int vfx_band_energy(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, int hop, double threshold, double* energy,
                    int* cut_bin, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(wav && cut_bin, "vfx_band_energy: NULL argument");
  VFX_CHECK(B > 0 && Lmax > 0, "vfx_band_energy: need B > 0 and Lmax > 0, got B=%d Lmax=%d", B, Lmax);
  VFX_CHECK(h->cfg.n_fft == 2048, "vfx_band_energy: needs the 44.1 kHz front end (n_fft 2048)");
  VFX_CHECK(hop >= 1 && hop <= h->cfg.n_fft, "vfx_band_energy: hop = %d (need 1 <= hop <= %d)", hop, h->cfg.n_fft);
  VFX_CHECK(threshold > 0.0 && threshold <= 1.0, "vfx_band_energy: threshold = %g (need 0 < threshold <= 1)", threshold);
  constexpr int kMaxFrames = 1 << 24;  // per clip: the groups of a launch set stay far inside 32 bits
  const int half = h->cfg.n_fft / 2;
  std::vector<int> host(B);
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    const int Lb = lengths ? lengths[b] : Lmax;
    VFX_CHECK(Lb > half && Lb <= Lmax, "vfx_band_energy: clip %d has %d samples (need %d < length <= Lmax = %d: reflect padding)", b, Lb,
              half, Lmax);
    VFX_CHECK(Lb <= 0x7fffffff - 2 * h->cfg.n_fft && Lb / hop + 1 <= kMaxFrames,
              "vfx_band_energy: clip %d has %d samples, %d frames at hop %d (at most %d frames)", b, Lb, Lb / hop + 1, hop, kMaxFrames);
    host[b] = Lb;
    longest = std::max(longest, Lb);
  }
  // the group partials of a launch set: at most kBandMaxClips clips, and fewer while a set of them would pass 256 MB
  const int groups = band_groups(longest, hop);
  const size_t clip_bytes = (size_t)groups * VFX_BAND_BINS * sizeof(double);
  const int step = (int)std::max<size_t>(1, std::min<size_t>(std::min(B, kBandMaxClips), ((size_t)256 << 20) / clip_bytes));
  double* const ws = reinterpret_cast<double*>(h->scratch.ensure(
      h, (size_t)step * clip_bytes, 8, "the varlen scratch would have to grow from %zu to %zu bytes, but a hipGraph was captured from plan "
      "'%s': run the largest vfx_band_energy batch once BEFORE capturing"));
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int b0 = 0; b0 < B; b0 += step) {  // (a clip's numbers do not depend on the launch it is in)
    const int n = std::min(step, B - b0);
    launch_band_energy(h->fe, wav + (int64_t)b0 * Lmax, n, Lmax, host.data() + b0, hop, threshold, groups, ws,
                       slice_rows(energy, b0, VFX_BAND_BINS), cut_bin + b0, s);
  }
  VFX_API_END
}

int vfx_mel_project(vfx_handle* h, const float* sp, int64_t rows, float* mel, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(sp && mel && rows > 0, "bad argument");
  launch_mel_project(h->fe, sp, rows, mel, static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_spectral_metrics(vfx_handle* h, const float* est, const float* target, int B, int T, int F, float* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(est && target && out && B > 0 && T > 0 && F > 0 && B <= 65535, "bad argument");
  // per-frame partial sums live in the arena (no plan is running concurrently: single stream, single thread)
  Plan tmp;
  tmp.arena_bytes = (size_t)B * T * 4 * sizeof(double);
  if (tmp.arena_bytes > h->arena.bytes) h->plans.clear();  // plans hold absolute pointers into the old arena
  bind_plan(h, tmp);
  launch_spectral_metrics(est, target, B, T, F, reinterpret_cast<double*>(h->arena.p), out, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// AudioMetrics.evaluation (score.hip)
// ---------------------------------------------------------------------------------------------
// byte offsets of vfx_audio_metrics' workspace for n clips of at most T frames and nslab SI-SDR slabs
struct ScoreLayout {
  size_t sp[2], mel[2], fr[2], ss[2], sisdr, end;
};
static ScoreLayout score_layout(int n, int T, int nslab, int nbins, int nmels) {
  auto up = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  ScoreLayout l{};
  const size_t nsp = (size_t)n * T * nbins * sizeof(float), nmel = (size_t)n * T * nmels * sizeof(float);
  const size_t nfr = (size_t)n * T * 7 * sizeof(double);
  size_t o = 0;
  for (int i = 0; i < 2; ++i) l.sp[i] = o, o += up(nsp);
  for (int i = 0; i < 2; ++i) l.mel[i] = o, o += up(nmel);
  for (int i = 0; i < 2; ++i) l.fr[i] = o, o += up(nfr);
  l.ss[0] = o, o += up((size_t)n * ssim_tiles(T, nbins) * sizeof(double));
  l.ss[1] = o, o += up((size_t)n * ssim_tiles(T, nmels) * sizeof(double));
  l.sisdr = o, o += up((size_t)n * nslab * 3 * sizeof(double));
  l.end = o;
  return l;
}

// the front end of a rate: the images' shapes, the frame rule and the shortest clip (7 frames: the smallest image skimage's 7 x 7
// SSIM accepts)
struct ScoreFrontEnd {
  int rate, hop, nbins, nmels, min_len;
  int frames(int len) const { return rate == kDftRate ? dft_frames(len) : len / hop + 1; }
};
static ScoreFrontEnd score_front_end(const vfx_handle* h, int rate, const char* who) {
  VFX_CHECK(rate == 44100 || rate == kDftRate, "%s: rate %d is not scored (the supported rates are 44100 and 16000)", who, rate);
  if (rate == kDftRate) return {rate, kDftHop, kDftBins, kDftMels, kDftMinLen};  // (its tables are its own: any handle has them)
  VFX_CHECK(h->cfg.n_fft == 2048 && h->cfg.n_mels == 128, "%s: needs the 44.1 kHz front end (n_fft 2048, 128 mel bands)", who);
  return {rate, h->cfg.hop, h->cfg.n_fft / 2 + 1, h->cfg.n_mels, 6 * h->cfg.hop};
}
// librosa.stft magnitudes (eps 0) and their mel projection, every clip framed at its own length; rows past it are zeros
static void launch_score_images(vfx_handle* h, const ScoreFrontEnd& fe, const float* wav, int n, int Lmax, int T, const int* d_lens,
                                float* sp, float* mel, hipStream_t s) {
  if (fe.rate == kDftRate)
    launch_stft_dft(ensure_score16k_tables(h), wav, n, Lmax, T, d_lens, sp, mel, s);
  else
    launch_stft_mel(h->fe, wav, n, Lmax, T, mel, sp, nullptr, nullptr, 0, fe.hop, 0.f, s, d_lens);
}

int vfx_audio_metrics_rate(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int rate,
                           double* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(est && target && lengths && out && B > 0 && Lmax > 0, "vfx_audio_metrics: bad argument");
  const ScoreFrontEnd fe = score_front_end(h, rate, "vfx_audio_metrics");
  const int nbins = fe.nbins, nmels = fe.nmels;
  VFX_CHECK(rate != kDftRate || Lmax < (1 << 30), "vfx_audio_metrics: Lmax = %d is too long at 16 kHz (need < 2^30)", Lmax);
  for (int b = 0; b < B; ++b)
    VFX_CHECK(lengths[b] >= fe.min_len && lengths[b] <= Lmax, "vfx_audio_metrics: clip %d has %d samples (need %d <= length <= Lmax = %d)",
              b, lengths[b], fe.min_len, Lmax);
  // sub-batches of consecutive clips: each as many as keep its workspace (spectra of ITS longest clip) under the cap
  struct Sub { int b0, n, T, nslab; };
  std::vector<Sub> subs;
  size_t need = 0;
  for (int b0 = 0; b0 < B;) {
    Sub s{b0, 0, 0, 0};
    while (b0 + s.n < B && s.n < kMaxVarlenClips) {
      const int Tn = std::max(s.T, fe.frames(lengths[b0 + s.n])), nsn = std::max(s.nslab, sisdr_slabs(lengths[b0 + s.n]));
      if (s.n > 0 && score_layout(s.n + 1, Tn, nsn, nbins, nmels).end > kScoreWorkspaceBytes) break;
      s.T = Tn;
      s.nslab = nsn;
      ++s.n;
    }
    need = std::max(need, score_layout(s.n, s.T, s.nslab, nbins, nmels).end);
    subs.push_back(s);
    b0 += s.n;
  }
  char* const ws = h->score_ws.ensure(h, need, 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_l = h->lens_row(LENS_SCORE_SAMPLES);
  int* const d_t = h->lens_row(LENS_SCORE_FRAMES);
  std::vector<int> frames(B);
  for (int b = 0; b < B; ++b) frames[b] = fe.frames(lengths[b]);
  for (const Sub& sb : subs) {
    const ScoreLayout l = score_layout(sb.n, sb.T, sb.nslab, nbins, nmels);
    auto f32 = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
    auto f64 = [&](size_t o) { return reinterpret_cast<double*>(ws + o); };
    launch_set_frames(d_l, lengths + sb.b0, sb.n, s);
    launch_set_frames(d_t, frames.data() + sb.b0, sb.n, s);
    const float* src[2] = {est + (int64_t)sb.b0 * Lmax, target + (int64_t)sb.b0 * Lmax};
    for (int i = 0; i < 2; ++i) launch_score_images(h, fe, src[i], sb.n, Lmax, sb.T, d_l, f32(l.sp[i]), f32(l.mel[i]), s);
    launch_sisdr_slabs(src[0], src[1], sb.n, Lmax, d_l, sb.nslab, f64(l.sisdr), s);
    launch_score_frames(f32(l.sp[0]), f32(l.sp[1]), sb.n, sb.T, nbins, d_t, f64(l.fr[0]), s);
    launch_score_frames(f32(l.mel[0]), f32(l.mel[1]), sb.n, sb.T, nmels, d_t, f64(l.fr[1]), s);
    launch_ssim_tiles(f32(l.sp[0]), f32(l.sp[1]), sb.n, sb.T, nbins, d_t, f64(l.ss[0]), s);
    launch_ssim_tiles(f32(l.mel[0]), f32(l.mel[1]), sb.n, sb.T, nmels, d_t, f64(l.ss[1]), s);
    ScoreFinalArgs a;
    a.lens = d_l;
    a.frames = d_t;
    a.sisdr_ws = f64(l.sisdr);
    a.nslab = sb.nslab;
    a.frames_ws[0] = f64(l.fr[0]);
    a.frames_ws[1] = f64(l.fr[1]);
    a.T = sb.T;
    a.ssim_ws[0] = f64(l.ss[0]);
    a.ssim_ws[1] = f64(l.ss[1]);
    a.ssim_stride[0] = ssim_tiles(sb.T, nbins);
    a.ssim_stride[1] = ssim_tiles(sb.T, nmels);
    a.F[0] = nbins;
    a.F[1] = nmels;
    a.out = out + (int64_t)sb.b0 * VFX_N_AUDIO_METRICS;
    launch_score_final(a, sb.n, s);
  }
  VFX_API_END
}

int vfx_audio_metrics(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, double* out,
                      void* stream) {
  return vfx_audio_metrics_rate(h, est, target, B, Lmax, lengths, 44100, out, stream);
}

int vfx_stoi(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int up, int down,
             const double* taps, int ntaps, double* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  stoi_scores(h, est, target, B, Lmax, lengths, up, down, taps, ntaps, out, nullptr, static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_bsseval(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int flen, double* out,
                void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  bsseval_scores(h, est, target, B, Lmax, lengths, flen, out, nullptr, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// validation losses (tools/pytorch/losses.py L1, L1_Sp, L1_Log_Sp on the device: losses.hip)
// ---------------------------------------------------------------------------------------------
int vfx_spec_losses(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, double* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(est && target && out, "vfx_spec_losses: NULL argument");
  VFX_CHECK(B > 0 && Lmax > 0, "vfx_spec_losses: need B > 0 and Lmax > 0, got B=%d Lmax=%d", B, Lmax);
  VFX_CHECK(h->cfg.n_fft == 2048, "vfx_spec_losses: needs the 44.1 kHz front end (n_fft 2048)");
  const int hop = h->cfg.hop, half = h->cfg.n_fft / 2, nbins = half + 1;
  std::vector<int> host(2 * (size_t)B);  // samples | frames
  for (int b = 0; b < B; ++b) {
    const int Lb = lengths ? lengths[b] : Lmax;
    VFX_CHECK(Lb > half && Lb <= Lmax, "vfx_spec_losses: clip %d has %d samples (need %d < length <= Lmax = %d: reflect padding)", b, Lb, half,
              Lmax);
    host[b] = Lb;
    host[(size_t)B + b] = Lb / hop + 1;
  }
  const int T = frames_of(h, Lmax), nchunk = l1_chunks(Lmax);
  const int step = std::min(B, kLossMaxClips);
  const size_t frame_bytes = (size_t)step * T * 2 * sizeof(double);
  char* const sc = h->scratch.ensure(h, frame_bytes + (size_t)step * nchunk * sizeof(double), 8,
                                     "the varlen scratch would have to grow from %zu to %zu bytes, but a hipGraph was captured from plan "
                                     "'%s': run the largest vfx_spec_losses batch once BEFORE capturing");
  double* const frame_ws = reinterpret_cast<double*>(sc);
  double* const chunk_ws = reinterpret_cast<double*>(sc + frame_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_n = h->lens_row(LENS_LOSS_COUNT);
  int* const d_f = h->lens_row(LENS_LOSS_FRAMES);
  for (int b0 = 0; b0 < B; b0 += step) {  // (a clip's numbers do not depend on the launch it is in)
    const int n = std::min(step, B - b0);
    const float* const e = est + (int64_t)b0 * Lmax;
    const float* const t = target + (int64_t)b0 * Lmax;
    launch_set_frames(d_n, host.data() + b0, n, s);
    launch_set_frames(d_f, host.data() + B + b0, n, s);
    launch_l1_rows(e, t, n, Lmax, d_n, nchunk, chunk_ws, s);
    launch_pair_stft_l1(h->fe, e, t, n, Lmax, T, d_n, hop, 1e-8f, frame_ws, s);
    launch_loss_final(chunk_ws, nchunk, d_n, frame_ws, T, d_f, nbins, 1, out + (int64_t)b0 * VFX_N_SPEC_LOSSES, VFX_N_SPEC_LOSSES, n, s);
  }
  VFX_API_END
}

int vfx_l1_rows(vfx_handle* h, const float* a, const float* b, int B, int64_t ld, const int* counts, double* out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(a && b && out, "vfx_l1_rows: NULL argument");
  VFX_CHECK(B > 0 && ld > 0 && ld <= 0x7fffffff, "vfx_l1_rows: need B > 0 and 0 < ld < 2^31, got B=%d ld=%lld", B, (long long)ld);
  std::vector<int> host(B);
  for (int r = 0; r < B; ++r) {
    host[r] = counts ? counts[r] : (int)ld;
    VFX_CHECK(host[r] >= 1 && host[r] <= ld, "vfx_l1_rows: row %d has %d elements (need 1 <= count <= ld = %lld)", r, host[r], (long long)ld);
  }
  const int nchunk = l1_chunks(ld);
  const int step = std::min(B, kLossMaxClips);
  double* const chunk_ws = reinterpret_cast<double*>(h->scratch.ensure(
      h, (size_t)step * nchunk * sizeof(double), 8, "the varlen scratch would have to grow from %zu to %zu bytes, but a hipGraph was captured "
      "from plan '%s': run the largest vfx_l1_rows batch once BEFORE capturing"));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_n = h->lens_row(LENS_LOSS_COUNT);
  for (int r0 = 0; r0 < B; r0 += step) {
    const int n = std::min(step, B - r0);
    launch_set_frames(d_n, host.data() + r0, n, s);
    launch_l1_rows(a + (int64_t)r0 * ld, b + (int64_t)r0 * ld, n, ld, d_n, nchunk, chunk_ws, s);
    launch_loss_final(chunk_ws, nchunk, d_n, nullptr, 0, nullptr, 0, 0, out + r0, 1, n, s);
  }
  VFX_API_END
}

int vfx_chunk_gather(vfx_handle* h, const float* x, int B, int L, int win, int hop, int lead, int n_chunks,
                     float* chunks, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && chunks && B > 0 && L > 0 && win > 0 && hop > 0 && lead >= 0 && n_chunks > 0, "bad argument");
  VFX_CHECK(B <= 65535 && n_chunks <= 65535, "chunk grid too large");
  launch_chunk_gather(x, B, L, win, hop, lead, n_chunks, chunks, static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_chunk_ola(vfx_handle* h, const float* frames, const float* window, float scale, int B, int n_chunks, int win,
                  int hop, int lead, int L, float* y, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(frames && y && B > 0 && L > 0 && win > 0 && hop > 0 && lead >= 0 && n_chunks > 0, "bad argument");
  VFX_CHECK(B <= 65535, "batch too large");
  launch_chunk_ola(frames, window, scale, B, n_chunks, win, hop, lead, L, y, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// polyphase resampling (librosa.load(path, sr=44100) / scipy.signal.resample_poly on the device: resample.hip)
// ---------------------------------------------------------------------------------------------
int64_t vfx_resample_out_len(int64_t n_in, int up, int down) {
  ResamplePair p;
  if (n_in < 0 || !resample_reduce(up, down, &p) || (p.up != p.down && p.R == 0)) return -1;
  return resample_out_len(n_in, p);
}

int vfx_resample_window(int64_t n_in, int up, int down, int64_t o0, int64_t n, int64_t* k0, int64_t* k1) {
  VFX_API_BEGIN
  ResamplePair p;
  VFX_CHECK(resample_reduce(up, down, &p), "vfx_resample_window: bad rates %d/%d", up, down);
  VFX_CHECK(n_in >= 0 && o0 >= 0 && n >= 0 && k0 && k1, "vfx_resample_window: bad argument");
  resample_window(n_in, p, o0, n, k0, k1);
  VFX_API_END
}

int vfx_resample(vfx_handle* h, const float* x, int B, int64_t ldx, int64_t x0, int64_t Lx, const int64_t* lens_in, int up, int down,
                 const float* taps, int ntaps, float* y, int64_t ldy, int64_t o0, int64_t n_out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  ResamplePair p;
  VFX_CHECK(resample_reduce(up, down, &p), "vfx_resample: bad rates %d/%d", up, down);
  VFX_CHECK(p.up != p.down, "vfx_resample: up / down = %d / %d is the same rate (nothing to filter)", up, down);
  VFX_CHECK(p.R > 0, "vfx_resample: the filter of %d/%d (%d taps) does not fit the kernel's LDS budget", p.up, p.down, 2 * p.hl + 1);
  VFX_CHECK(ntaps == 2 * p.hl + 1, "vfx_resample: %d taps given, %d/%d needs 2*10*%d + 1 = %d", ntaps, p.up, p.down,
            std::max(p.up, p.down), 2 * p.hl + 1);
  VFX_CHECK(x && taps && y && lens_in && B > 0 && B <= 65535 * kResampleMaxClips, "vfx_resample: bad argument");
  VFX_CHECK(x0 >= 0 && Lx >= 0 && ldx >= Lx && o0 >= 0 && n_out > 0 && ldy >= n_out, "vfx_resample: bad window or row stride");
  for (int b = 0; b < B; ++b) {
    VFX_CHECK(lens_in[b] >= 0, "vfx_resample: clip %d has a negative length", b);
    int64_t k0, k1;
    resample_window(lens_in[b], p, o0, n_out, &k0, &k1);
    VFX_CHECK(k1 <= k0 || (x0 <= k0 && k1 <= x0 + Lx),
              "vfx_resample: clip %d: outputs [%lld, %lld) need input samples [%lld, %lld), the window holds [%lld, %lld)", b,
              (long long)o0, (long long)(o0 + n_out), (long long)k0, (long long)k1, (long long)x0, (long long)(x0 + Lx));
  }
  launch_resample(x, B, ldx, x0, Lx, lens_in, p, taps, y, ldy, o0, n_out, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// What every clip-batch entry point checks of its lengths before it launches anything: min_len <= lengths[b] <= ldx, <= *ldy (NULL: the
// operation has no second stride to hold a clip to), <= cap -- what the operation's kernels take in 32-bit indices.  `more_than` names
// what a minimum above 1 is one more than (sosfiltfilt's padlen); without it a clip below the minimum is empty, or negative where empty
// clips are taken.  -> the longest clip, or throws
static int64_t check_clip_lengths(const char* who, int B, const int64_t* lengths, int64_t min_len, const char* more_than, int64_t ldx,
                                  const int64_t* ldy, int64_t cap) {
  int64_t lmax = 0;
  for (int b = 0; b < B; ++b) {
    const long long n = lengths[b];
    if (more_than)
      VFX_CHECK(n >= min_len, "%s: clip %d has %lld samples: the length must be greater than %s, which is %lld", who, b, n, more_than,
                (long long)(min_len - 1));
    else if (min_len <= 0)
      VFX_CHECK(n >= min_len, "%s: clip %d has a negative length", who, b);
    else
      VFX_CHECK(n >= min_len, "%s: clip %d is empty (%lld samples)", who, b, n);
    if (!ldy)
      VFX_CHECK(n <= ldx && n <= cap, "%s: clip %d has %lld samples, the rows hold %lld", who, b, n, (long long)ldx);
    else
      VFX_CHECK(n <= ldx && n <= *ldy && n <= cap, "%s: clip %d has %lld samples, the rows hold %lld and %lld", who, b, n, (long long)ldx,
                (long long)*ldy);
    lmax = std::max(lmax, lengths[b]);
  }
  return lmax;
}

int64_t vfx_resample_each_out_len(int64_t n_in, int up, int down) {
  ResamplePair p;
  if (n_in < 0 || n_in > ((int64_t)1 << 46) || !resample_each_reduce(up, down, &p)) return -1;
  return resample_out_len(n_in, p);
}

int vfx_resample_each(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lens_in, const int* pair_index,
                      const int* up, const int* down, const void* taps, const int64_t* taps_at, int F, void* y, int64_t ldy, int64_t n_out,
                      void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lens_in && pair_index && up && down && taps && taps_at && y && (x_f64 == 0 || x_f64 == 1), "vfx_resample_each: bad argument");
  VFX_CHECK(B >= 1 && B <= kResampleEachMaxClips, "vfx_resample_each: %d clips (need 1 <= B <= %d)", B, kResampleEachMaxClips);
  VFX_CHECK(F >= 1 && F <= kResampleEachMaxDesigns, "vfx_resample_each: %d designs (need 1 <= F <= %d)", F, kResampleEachMaxDesigns);
  VFX_CHECK(n_out >= 0 && n_out <= ldy && n_out <= (int64_t)0x7fffffff * kResampleEachBlock && ldx >= 0,
            "vfx_resample_each: bad n_out (%lld) or row stride (%lld, %lld)", (long long)n_out, (long long)ldx, (long long)ldy);
  ResamplePair pairs[kResampleEachMaxDesigns];
  bool taken[kResampleEachMaxDesigns];
  for (int f = 0; f < F; ++f) {
    VFX_CHECK(up[f] > 0 && down[f] > 0, "vfx_resample_each: design %d: bad rates %d/%d", f, up[f], down[f]);
    taken[f] = resample_each_reduce(up[f], down[f], &pairs[f]);
    VFX_CHECK(!taken[f] || pairs[f].up == pairs[f].down || taps_at[f] >= 0, "vfx_resample_each: design %d: taps_at = %lld", f,
              (long long)taps_at[f]);
  }
  for (int b = 0; b < B; ++b) {
    const int f = pair_index[b];
    VFX_CHECK(f >= 0 && f < F, "vfx_resample_each: clip %d asks for design %d of %d", b, f, F);
    if (!taken[f]) {
      const int64_t g = std::gcd((int64_t)up[f], (int64_t)down[f]);
      VFX_CHECK(false, "vfx_resample_each: clip %d: the pair %lld/%lld (reduced) is past the cap max(up, down) <= %d", b,
                (long long)(up[f] / g), (long long)(down[f] / g), kResampleEachMaxRate);
    }
  }
  check_clip_lengths("vfx_resample_each", B, lens_in, 0, nullptr, ldx, nullptr, (int64_t)1 << 46);
  for (int f = 0; f < F; ++f)  // (a design past the cap that no clip asks for)
    VFX_CHECK(taken[f], "vfx_resample_each: design %d: the pair %d/%d is past the cap max(up, down) <= %d after the gcd", f, up[f], down[f],
              kResampleEachMaxRate);
  if (n_out > 0)
    launch_resample_each(h, x, x_f64, B, ldx, lens_in, pair_index, pairs, taps, taps_at, F, y, ldy, n_out, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// zero-phase IIR filter (scipy.signal.sosfiltfilt on the device: sosfilt.hip)
// ---------------------------------------------------------------------------------------------
int vfx_sosfiltfilt(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const double* sos, int S,
                    const double* zi, int padlen, double* y, int64_t ldy, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(S >= 1 && S <= kSosMaxSections, "vfx_sosfiltfilt: %d sections (need 1 <= S <= %d)", S, kSosMaxSections);
  VFX_CHECK(x && lengths && sos && zi && y && B > 0 && (x_f64 == 0 || x_f64 == 1), "vfx_sosfiltfilt: bad argument");
  VFX_CHECK(padlen >= 0 && padlen <= 3 * (2 * kSosMaxSections + 1), "vfx_sosfiltfilt: padlen %d (need 0 <= padlen <= %d)", padlen,
            3 * (2 * kSosMaxSections + 1));
  for (int i = 0; i < S; ++i) VFX_CHECK(sos[i * 6 + 3] == 1.0, "vfx_sosfiltfilt: sos[%d][3] = %g, should be 1", i, sos[i * 6 + 3]);
  const int64_t lmax = check_clip_lengths("vfx_sosfiltfilt", B, lengths, padlen + 1, "padlen", ldx, &ldy, 0x7fffffff - 1024);
  const int64_t ldf = (lmax + 2 * padlen + 63) / 64 * 64;
  double* const f = reinterpret_cast<double*>(h->sos_ws.ensure(h, (size_t)std::min(B, kSosMaxClips) * ldf * sizeof(double), 0));
  launch_sosfiltfilt(x, x_f64, B, ldx, lengths, sos, S, zi, padlen, f, ldf, y, ldy, static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_sosfiltfilt_bank(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* filter_index,
                         const double* sos, const double* zi, const int* sections, const int* padlens, int F, int Smax, double* y,
                         int64_t ldy, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && filter_index && sos && zi && sections && padlens && y && B > 0 && (x_f64 == 0 || x_f64 == 1),
            "vfx_sosfiltfilt_bank: bad argument");
  VFX_CHECK(F >= 1 && F <= kSosMaxDesigns, "vfx_sosfiltfilt_bank: %d designs (need 1 <= F <= %d)", F, kSosMaxDesigns);
  VFX_CHECK(Smax >= 1 && Smax <= kSosMaxSections, "vfx_sosfiltfilt_bank: rows of %d sections (need 1 <= Smax <= %d)", Smax, kSosMaxSections);
  for (int f = 0; f < F; ++f) {
    VFX_CHECK(sections[f] >= 1 && sections[f] <= Smax, "vfx_sosfiltfilt_bank: design %d has %d sections (need 1 <= S <= %d)", f, sections[f],
              Smax);
    VFX_CHECK(padlens[f] >= 0 && padlens[f] <= 3 * (2 * sections[f] + 1), "vfx_sosfiltfilt_bank: design %d: padlen %d (need 0 <= padlen <= %d)",
              f, padlens[f], 3 * (2 * sections[f] + 1));
    for (int i = 0; i < sections[f]; ++i)
      VFX_CHECK(sos[((size_t)f * Smax + i) * 6 + 3] == 1.0, "vfx_sosfiltfilt_bank: design %d: sos[%d][3] = %g, should be 1", f, i,
                sos[((size_t)f * Smax + i) * 6 + 3]);
  }
  check_clip_lengths("vfx_sosfiltfilt_bank", B, lengths, INT64_MIN, nullptr, ldx, &ldy, 0x7fffffff - 1024);  // (no common minimum:)
  int64_t lext = 0;
  for (int b = 0; b < B; ++b) {  // the minimum is the padlen of the clip's own design
    VFX_CHECK(filter_index[b] >= 0 && filter_index[b] < F, "vfx_sosfiltfilt_bank: clip %d asks for design %d of %d", b, filter_index[b], F);
    const int padlen = padlens[filter_index[b]];
    VFX_CHECK(lengths[b] > padlen,
              "vfx_sosfiltfilt_bank: clip %d has %lld samples: the length must be greater than padlen, which is %d for its design %d", b,
              (long long)lengths[b], padlen, filter_index[b]);
    lext = std::max(lext, lengths[b] + 2 * padlen);
  }
  const int64_t ldf = (lext + 63) / 64 * 64;
  double* const f = reinterpret_cast<double*>(h->sos_ws.ensure(h, (size_t)std::min(B, kSosMaxClips) * ldf * sizeof(double), 0));
  const size_t bank_bytes = (size_t)F * Smax * kSosBankRow * sizeof(double);
  sosfilt_pack_bank(sos, zi, F, Smax, reinterpret_cast<double*>(h->sos_bank.stage(h, bank_bytes)));
  const double* const bank = reinterpret_cast<const double*>(h->sos_bank.upload(bank_bytes, static_cast<hipStream_t>(stream)));
  launch_sosfiltfilt_bank(x, x_f64, B, ldx, lengths, filter_index, bank, Smax, sections, padlens, f, ldf, y, ldy,
                          static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// room-impulse-response convolution (MagicalEffects.reverb_rir on the device: reverb.hip)
// ---------------------------------------------------------------------------------------------
int vfx_reverb_rir(vfx_handle* h, const float* x, int B, int64_t ldx, const int64_t* lengths, const float* rirs, int R, int64_t ldr,
                   const int64_t* rir_lengths, const int* rir_index, int normalize, float* y, int64_t ldy, float* peaks, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && rirs && rir_lengths && y && B > 0 && R > 0, "vfx_reverb_rir: bad argument");
  VFX_CHECK(peaks || !normalize, "vfx_reverb_rir: peaks may be NULL only when normalize is 0");
  for (int r = 0; r < R; ++r) {
    VFX_CHECK(rir_lengths[r] >= 1, "vfx_reverb_rir: RIR %d is empty (%lld taps)", r, (long long)rir_lengths[r]);
    VFX_CHECK(rir_lengths[r] <= kReverbMaxTaps, "vfx_reverb_rir: RIR %d has %lld taps, at most %d are taken", r, (long long)rir_lengths[r],
              kReverbMaxTaps);
    VFX_CHECK(rir_lengths[r] <= ldr, "vfx_reverb_rir: RIR %d has %lld taps, the rows hold %lld", r, (long long)rir_lengths[r], (long long)ldr);
  }
  const int64_t lmax = check_clip_lengths("vfx_reverb_rir", B, lengths, 1, nullptr, ldx, nullptr, 0x7fffffff - kReverbMaxTaps - 2 * kReverbTile);
  for (int b = 0; rir_index && b < B; ++b)
    VFX_CHECK(rir_index[b] >= 0 && rir_index[b] < R, "vfx_reverb_rir: clip %d asks for RIR %d of %d", b, rir_index[b], R);
  VFX_CHECK(ldy >= lmax, "vfx_reverb_rir: ldy = %lld is too small for a clip of %lld samples", (long long)ldy, (long long)lmax);
  launch_reverb_rir(x, B, ldx, lengths, rirs, ldr, rir_lengths, rir_index, R, normalize, y, ldy, peaks, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// noise mixing (add_noise_and_scale, _with_HQ, _with_HQ_with_Aug on the device: mix.hip)
// ---------------------------------------------------------------------------------------------
int vfx_mix_noise(vfx_handle* h, int form, int B, int64_t ld, const int64_t* lengths, const float* front, const float* noise,
                  const float* hq, const float* aug, const double* noise_weight, const double* scale, float* front_out, float* noise_out,
                  float* hq_out, float* aug_out, float* noisy, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(form >= 0 && form <= 2, "vfx_mix_noise: form %d (0 = plain, 1 = with HQ, 2 = with HQ and Aug)", form);
  VFX_CHECK(front && noise && lengths && scale && B > 0, "vfx_mix_noise: bad argument");
  VFX_CHECK(B <= kMaxVarlenClips, "vfx_mix_noise: %d clips, at most %d per call", B, kMaxVarlenClips);
  VFX_CHECK((form >= 1) == (hq != nullptr), "vfx_mix_noise: form %d %s hq", form, form >= 1 ? "needs" : "takes no");
  VFX_CHECK((form == 2) == (aug != nullptr), "vfx_mix_noise: form %d %s aug (aug goes with hq: form 2)", form, form == 2 ? "needs" : "takes no");
  VFX_CHECK((hq || !hq_out) && (aug || !aug_out), "vfx_mix_noise: form %d returns no %s", form, hq_out && !hq ? "hq" : "aug");
  VFX_CHECK(front_out || noise_out || hq_out || aug_out || noisy, "vfx_mix_noise: no output asked for");
  const int64_t lmax = check_clip_lengths("vfx_mix_noise", B, lengths, 1, nullptr, ld, nullptr, 0x7fffffff - 2 * kClipChunk);
  char* const ws = h->mix_ws.ensure(h, mix_workspace_bytes(B, lmax), 0);
  const float* const in[4] = {front, noise, hq, aug};
  float* const out[5] = {front_out, noise_out, hq_out, aug_out, noisy};
  launch_mix_noise(form, B, ld, lengths, in, noise_weight, scale, out, ws, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// array effects (MagicalEffects.quantification and time_dropout on the device: effects.hip)
// ---------------------------------------------------------------------------------------------
int vfx_quantize(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* bins, double* y,
                 int64_t ldy, void* peaks, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && bins && y && (x_f64 == 0 || x_f64 == 1), "vfx_quantize: bad argument");
  VFX_CHECK(B >= 1 && B <= kMaxVarlenClips, "vfx_quantize: %d clips (need 1 <= B <= %d)", B, kMaxVarlenClips);
  check_clip_lengths("vfx_quantize", B, lengths, 1, nullptr, ldx, &ldy, 0x7fffffff - 2 * kClipChunk);
  for (int b = 0; b < B; ++b)
    VFX_CHECK(bins[b] >= 0 && bins[b] <= kFxMaxBins, "vfx_quantize: clip %d: %d bins (need 0 <= bins <= %d)", b, bins[b], kFxMaxBins);
  auto* const bits = reinterpret_cast<unsigned long long*>(h->fx_ws.ensure(h, (size_t)kMaxVarlenClips * sizeof(unsigned long long), 0));
  launch_quantize(x, x_f64, B, ldx, lengths, bins, y, ldy, peaks, bits, static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_time_dropout(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int64_t* starts,
                     const int64_t* ends, const double* smooth, void* y, int64_t ldy, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && starts && ends && smooth && y && (x_f64 == 0 || x_f64 == 1), "vfx_time_dropout: bad argument");
  VFX_CHECK(B >= 1 && B <= kMaxVarlenClips, "vfx_time_dropout: %d clips (need 1 <= B <= %d)", B, kMaxVarlenClips);
  check_clip_lengths("vfx_time_dropout", B, lengths, 1, nullptr, ldx, &ldy, 0x7fffffff - 2 * kClipChunk);
  for (int b = 0; b < B; ++b)
    VFX_CHECK(starts[b] >= 0 && ends[b] >= starts[b], "vfx_time_dropout: clip %d: bad range [%lld, %lld) (need 0 <= start <= end)", b,
              (long long)starts[b], (long long)ends[b]);
  constexpr size_t kSmooth = (size_t)kFxSmoothRows * kFxSmoothKnots;
  if (h->fx_smooth_seen.size() != kSmooth || memcmp(h->fx_smooth_seen.data(), smooth, kSmooth * sizeof(double)) != 0) {
    memcpy(h->fx_smooth.stage(h, kSmooth * sizeof(double)), smooth, kSmooth * sizeof(double));
    h->fx_smooth.upload(kSmooth * sizeof(double), static_cast<hipStream_t>(stream));
    h->fx_smooth_seen.assign(smooth, smooth + kSmooth);
  }
  launch_time_dropout(x, x_f64, B, ldx, lengths, starts, ends, reinterpret_cast<const double*>(h->fx_smooth.dev.p), y, ldy,
                      static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// effect chain (the biquads, clip and reverse of MagicalEffects' sox chain on the device: chain.hip)
// ---------------------------------------------------------------------------------------------
int vfx_effect_chain(vfx_handle* h, const float* x, int B, int64_t ldx, const int64_t* lengths, const int* ops, const double* coef, int K,
                     float* y, int64_t ldy, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && ops && coef && y, "vfx_effect_chain: bad argument");
  VFX_CHECK(B >= 1 && B <= kMaxVarlenClips, "vfx_effect_chain: %d clips (need 1 <= B <= %d)", B, kMaxVarlenClips);
  VFX_CHECK(K >= 1 && K <= kChainMaxOps, "vfx_effect_chain: programs of %d steps (need 1 <= K <= %d)", K, kChainMaxOps);
  const int64_t lmax = check_clip_lengths("vfx_effect_chain", B, lengths, 1, nullptr, ldx, &ldy, 0x7fffffff - 2 * kClipChunk);
  std::vector<ChainPass> passes;
  std::vector<int> first;
  chain_plan(B, lengths, ops, coef, K, passes, first);
  bool uses[2] = {false, false};  // the scratch rows the passes name
  for (const ChainPass& p : passes)
    for (int i = 0; i < 2; ++i) uses[i] |= p.dst == CHAIN_BUF0 + i;
  constexpr size_t kStats = (size_t)kChainMaxClips * kChainMaxPasses * 2 * sizeof(unsigned);
  static_assert(kStats % 16 == 0, "the scratch rows behind the statistics stay 16-byte aligned");
  const int64_t lds = (lmax + 3) / 4 * 4;
  const size_t buf_bytes = (size_t)std::min(B, kChainMaxClips) * lds * sizeof(double);
  char* const ws = h->chain_ws.ensure(h, kStats + ((size_t)uses[0] + uses[1]) * buf_bytes, 0);
  double* const buf0 = uses[0] ? reinterpret_cast<double*>(ws + kStats) : nullptr;
  double* const buf1 = uses[1] ? reinterpret_cast<double*>(ws + kStats + (uses[0] ? buf_bytes : 0)) : nullptr;
  const size_t tab_bytes = passes.size() * sizeof(ChainPass);
  memcpy(h->chain_tab.stage(h, tab_bytes), passes.data(), tab_bytes);
  const ChainPass* const tab = reinterpret_cast<const ChainPass*>(h->chain_tab.upload(tab_bytes, static_cast<hipStream_t>(stream)));
  launch_effect_chain(x, ldx, B, passes, first, tab, buf0, buf1, lds, reinterpret_cast<unsigned*>(ws), y, ldy,
                      static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// silence and activity (tools/others/audio_op.py:79-150 on the device: activity.hip)
// ---------------------------------------------------------------------------------------------
// What the three entry points share once their own arguments are checked: the lengths, the threshold in the clips' dtype, the peaks'
// scratch, the launches.
static void run_activity(vfx_handle* h, const char* who, int mode, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths,
                         int64_t W, int64_t S, double threshold, int64_t* start, int64_t* stop, int* flag, uint8_t* labels, int64_t ldf,
                         int64_t* counts, void* stream) {
  VFX_CHECK(x_f64 == 0 || x_f64 == 1, "%s: x_f64 = %d (need 0 or 1)", who, x_f64);
  VFX_CHECK(B >= 1 && B <= kMaxVarlenClips, "%s: %d clips (need 1 <= B <= %d)", who, B, kMaxVarlenClips);
  VFX_CHECK(std::isfinite(threshold), "%s: threshold = %g (need a finite number)", who, threshold);
  if (mode == ACT_FRAMES)
    check_clip_lengths(who, B, lengths, S + 1, "the reflect padding", ldx, nullptr, 0x7fffffff - 2 * kClipChunk);
  else
    check_clip_lengths(who, B, lengths, 0, nullptr, ldx, nullptr, 0x7fffffff - 2 * kClipChunk);
  int64_t ldp = 1;
  for (int b = 0; b < B; ++b) {
    const int64_t c = activity_windows(mode, lengths[b], W, S);
    if (mode == ACT_FRAMES) VFX_CHECK(c <= ldf, "%s: clip %d has %lld frames, the label rows hold %lld", who, b, (long long)c, (long long)ldf);
    ldp = std::max(ldp, c);
  }
  const size_t esz = x_f64 ? sizeof(double) : sizeof(float);
  void* const ws = h->scratch.ensure(
      h, (size_t)(mode == ACT_BOTH ? 2 : 1) * std::min(B, kActMaxClips) * ldp * esz, 8,
      "the varlen scratch would have to grow from %zu to %zu bytes, but a hipGraph was captured from plan '%s': run the largest silence / "
      "activity batch once BEFORE capturing");
  // a Python scalar against a float32 array is compared in float32 (NumPy >= 2): the threshold is rounded once, here
  const double thr = x_f64 ? threshold : (double)(float)threshold;
  launch_activity(mode, x, x_f64, B, ldx, lengths, W, S, thr, ws, ldp, start, stop, flag, labels, ldf, counts,
                  static_cast<hipStream_t>(stream));
}

int vfx_trim_bounds(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, int64_t seg, double threshold,
                    int which, int64_t* start, int64_t* stop, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && start && stop, "vfx_trim_bounds: NULL argument");
  VFX_CHECK(seg > 0, "vfx_trim_bounds: seg = %lld (need seg > 0)", (long long)seg);
  VFX_CHECK(which == VFX_TRIM_TAIL || which == VFX_TRIM_HEAD || which == VFX_TRIM_BOTH, "vfx_trim_bounds: which = %d (need VFX_TRIM_TAIL, "
            "VFX_TRIM_HEAD or VFX_TRIM_BOTH)", which);
  static_assert(VFX_TRIM_TAIL == ACT_TAIL && VFX_TRIM_HEAD == ACT_HEAD && VFX_TRIM_BOTH == ACT_BOTH, "the public names of the modes");
  run_activity(h, "vfx_trim_bounds", which, x, x_f64, B, ldx, lengths, seg, seg, threshold, start, stop, nullptr, nullptr, 0, nullptr,
               stream);
  VFX_API_END
}

int vfx_long_empty(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, int64_t seg, int64_t step,
                   double threshold, int* flag, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && flag, "vfx_long_empty: NULL argument");
  VFX_CHECK(seg > 0 && step > 0, "vfx_long_empty: seg = %lld, step = %lld (need both > 0)", (long long)seg, (long long)step);
  run_activity(h, "vfx_long_empty", ACT_LONG, x, x_f64, B, ldx, lengths, seg, step, threshold, nullptr, nullptr, flag, nullptr, 0,
               nullptr, stream);
  VFX_API_END
}

int64_t vfx_active_frames_count(int64_t n, int64_t frame, int64_t shift) {
  if (n < 0 || frame <= 0 || shift <= 0 || n > 0x7fffffff || shift > 0x7fffffff) return -1;
  return activity_windows(ACT_FRAMES, n, frame, shift);
}

int vfx_active_frames(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, int64_t frame, int64_t shift,
                      double threshold, uint8_t* labels, int64_t ldf, int64_t* counts, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(x && lengths && labels, "vfx_active_frames: NULL argument");
  VFX_CHECK(frame > 0 && shift > 0 && shift <= 0x7fffffff, "vfx_active_frames: frame = %lld, shift = %lld (need both > 0)",
            (long long)frame, (long long)shift);
  VFX_CHECK(ldf >= 1, "vfx_active_frames: ldf = %lld (need ldf >= 1)", (long long)ldf);
  run_activity(h, "vfx_active_frames", ACT_FRAMES, x, x_f64, B, ldx, lengths, frame, shift, threshold, nullptr, nullptr, nullptr, labels,
               ldf, counts, stream);
  VFX_API_END
}

int vfx_istft(vfx_handle* h, const float* re, const float* im, int B, int T, int L, float* wav, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(re && im && wav && B > 0 && T > 0 && L > 0, "bad argument");
  launch_istft(h->fe, re, im, B, T, L, h->cfg.hop, wav, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// model stages
// ---------------------------------------------------------------------------------------------
static BufRef ext(int slot) {
  BufRef b;
  b.ext = true;
  b.slot = slot;
  return b;
}
static BufRef arena_buf(size_t off) {
  BufRef b;
  b.off = off;
  return b;
}

size_t vfx_workspace_bytes(vfx_handle* h, int model, int B, int T) {
  try {
    if (!h) return 0;
    DeviceGuard device_guard_(h->device);
    Plan plan;
    PlanBuilder pb{h, &plan, {}};
    if (model == VFX_MODEL_UNET_MEL) build_unet_mel(pb, B, T, ext(0), ext(1));
    else if (model == VFX_MODEL_UNET_SPEC) build_unet_spec(pb, B, T, ext(0), ext(1), ext(2), ext(3), ext(4));
    else if (model == VFX_MODEL_VOCODER) build_vocoder(pb, B, T, ext(0), ext(1));
    else if (model == VFX_MODEL_GRU_MEL || model == VFX_MODEL_DNN_MEL) build_analysis_mel(pb, model, B, T, ext(0), ext(1));
    else return 0;
    return pb.arena.high;
  } catch (...) {
    return 0;
  }
}

int vfx_reserve(vfx_handle* h, int model, int B, int T) {
  VFX_API_BEGIN_H(h)
  const size_t need = vfx_workspace_bytes(h, model, B, T);
  VFX_CHECK(need > 0, "vfx_reserve: cannot plan model %d (weights finalized?): %s", model, vfx_last_error());
  Plan tmp;
  tmp.arena_bytes = need;
  bind_plan(h, tmp);
  VFX_API_END
}

// The convolution kernels address a tensor with 32-bit byte offsets (buffer descriptors, LDS-DMA), so one
// launch handles tensors below 4 GiB.  A batch whose largest activation would exceed that is run as
// consecutive sub-batches on the same stream (clips are independent; each sub-batch re-uses the cached plan).
// Largest activation per clip: ResUNet level 1 (Tpad x W x 32 ch) and the vocoder's widest-in-bytes stack.
static int max_clips_per_launch(const vfx_handle* h, int T, bool unet_mel, bool unet_spec, bool voc) {
  const int64_t Tpad = (T + 63) / 64 * 64;
  int64_t per_clip = 1;
  if (unet_mel) per_clip = std::max<int64_t>(per_clip, Tpad * 127 * 64 * 4);      // cat(up, skip) of 2 x 32 channels
  if (unet_spec) per_clip = std::max<int64_t>(per_clip, Tpad * 1024 * 64 * 4);
  if (voc) {
    int64_t len = T + T % 2 + 4, c = h->cfg.voc_channels;
    per_clip = std::max(per_clip, len * c * 4);
    for (int i = 0; i < h->cfg.voc_n_stages; ++i) {
      len *= h->cfg.voc_scales[i];
      c /= 2;
      per_clip = std::max(per_clip, len * c * 4);
    }
  }
  int64_t lim = (((int64_t)1 << 32) - (1 << 20)) / per_clip;
  if (const char* e = getenv("VFX_MAX_CLIPS")) lim = std::min<int64_t>(lim, atoi(e));  // tests: force the sub-batch path
  return (int)std::max<int64_t>(1, std::min<int64_t>(lim, 1 << 20));
}

static int vfx_resunet_mel_1(vfx_handle* h, const float* mel_linear, int B, int T, float* logmel_out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(mel_linear && logmel_out && B > 0 && T > 0, "bad argument");
  VFX_CHECK(h->unet[VFX_MODEL_UNET_MEL], "vfx_resunet_mel: weights of the mel ResUNet are not finalized");
  run_plan(h, key_of("unet_mel", B, T), stream, {mel_linear, logmel_out},
           [&](PlanBuilder& pb) { build_unet_mel(pb, B, T, ext(0), ext(1)); });
  VFX_API_END
}
int vfx_resunet_mel(vfx_handle* h, const float* mel_linear, int B, int T, float* logmel_out, void* stream) {
  if (!h || B <= 0 || T <= 0) return vfx_resunet_mel_1(h, mel_linear, B, T, logmel_out, stream);
  return for_sub_batches(B, max_clips_per_launch(h, T, true, false, false), [&](int b, int n) {
    return vfx_resunet_mel_1(h, mel_linear + (int64_t)b * T * 128, n, T, logmel_out + (int64_t)b * T * 128, stream);
  });
}

// Generator.forward with the bi_gru / dnn module (analysis.hip); the ResUNet goes through vfx_resunet_mel.  frames (HOST) are copied
// into a row of their own of the handle's per-clip table (LENS_ANALYSIS_FRAMES), in stream order, for kMaxVarlenClips clips per launch set.
static int vfx_analysis_mel_1(vfx_handle* h, int model, const float* mel_linear, int B, int T, const int* frames, float* logmel_out,
                              void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(mel_linear && logmel_out && B > 0 && T > 0, "bad argument");
  VFX_CHECK(h->analysis[model - VFX_MODEL_GRU_MEL], "vfx_analysis_mel: weights of the %s module are not finalized",
            model == VFX_MODEL_GRU_MEL ? "bi_gru" : "dnn");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_f = h->lens_row(LENS_ANALYSIS_FRAMES);
  if (frames) {
    for (int b = 0; b < B; ++b)
      VFX_CHECK(frames[b] >= 1 && frames[b] <= T, "vfx_analysis_mel: clip %d has %d frames (need 1 <= frames <= T = %d)", b, frames[b], T);
    launch_set_frames(d_f, frames, B, s);
  }
  run_plan(h, key_of(model == VFX_MODEL_GRU_MEL ? "gru_mel" : "dnn_mel", B, T, frames ? 1 : 0), stream, {mel_linear, logmel_out},
           [&](PlanBuilder& pb) {
             if (frames) pb.lens_t = d_f;
             build_analysis_mel(pb, model, B, T, ext(0), ext(1));
           });
  VFX_API_END
}

int vfx_analysis_mel(vfx_handle* h, int model, const float* mel_linear, int B, int T, const int* frames, float* logmel_out,
                     void* stream) {
  if (model == VFX_MODEL_UNET_MEL) {
    if (frames) {
      set_error("vfx_analysis_mel: the ResUNet takes no per-clip frame counts (frames must be NULL)");
      return 1;
    }
    return vfx_resunet_mel(h, mel_linear, B, T, logmel_out, stream);
  }
  if (model != VFX_MODEL_GRU_MEL && model != VFX_MODEL_DNN_MEL) {
    set_error("vfx_analysis_mel: model %d is not an analysis module", model);
    return 1;
  }
  if (!h || B <= 0 || T <= 0) return vfx_analysis_mel_1(h, model, mel_linear, B, T, frames, logmel_out, stream);
  return for_sub_batches(B, kMaxVarlenClips, [&](int b, int n) {
    return vfx_analysis_mel_1(h, model, mel_linear + (int64_t)b * T * 128, n, T, frames ? frames + b : nullptr,
                              logmel_out + (int64_t)b * T * 128, stream);
  });
}

int vfx_select_analysis(vfx_handle* h, int model) {
  VFX_API_BEGIN_H(h)
  if (model == VFX_MODEL_UNET_MEL) {
    VFX_CHECK(h->unet[VFX_MODEL_UNET_MEL], "vfx_select_analysis: weights of the mel ResUNet are not finalized");
  } else {
    VFX_CHECK(model == VFX_MODEL_GRU_MEL || model == VFX_MODEL_DNN_MEL, "vfx_select_analysis: model %d is not an analysis module", model);
    VFX_CHECK(h->analysis[model - VFX_MODEL_GRU_MEL], "vfx_select_analysis: weights of the %s module are not finalized",
              model == VFX_MODEL_GRU_MEL ? "bi_gru" : "dnn");
  }
  h->analysis_model = model;
  VFX_API_END
}

static int vfx_resunet_spec_1(vfx_handle* h, const float* sp, const float* wav, int B, int T, int L, float* wav_out,
                              void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(sp && wav && wav_out && B > 0 && T > 0, "bad argument");
  VFX_CHECK(h->unet[VFX_MODEL_UNET_SPEC], "vfx_resunet_spec: weights of the spectrogram ResUNet are not finalized");
  VFX_CHECK(T == frames_of(h, L), "vfx_resunet_spec: T=%d does not match L=%d (expected %d frames)", T, L, frames_of(h, L));
  const size_t nsp = (size_t)B * T * (h->cfg.n_fft / 2 + 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto arena_f = [h](size_t off) { return reinterpret_cast<float*>(h->arena.p + off); };
  auto plan = run_plan(h, key_of("unet_spec", B, T), stream, {sp}, [&](PlanBuilder& pb) {
    auto& nm = pb.plan->named;
    nm["cos"] = pb.alloc_f(nsp);
    nm["sin"] = pb.alloc_f(nsp);
    nm["re"] = pb.alloc_f(nsp);
    nm["im"] = pb.alloc_f(nsp);
    build_unet_spec(pb, B, T, ext(0), arena_buf(nm["cos"]), arena_buf(nm["sin"]), arena_buf(nm["re"]), arena_buf(nm["im"]));
  }, [&](Plan& pl) {
    // second STFT of the same audio for the phase (unet_v2.py:96)
    launch_stft_mel(h->fe, wav, B, L, T, nullptr, nullptr, arena_f(pl.named["cos"]), arena_f(pl.named["sin"]), 0, h->cfg.hop, 1e-8f, s);
  });
  launch_istft(h->fe, arena_f(plan->named["re"]), arena_f(plan->named["im"]), B, T, L, h->cfg.hop, wav_out, s);
  VFX_API_END
}
int vfx_resunet_spec(vfx_handle* h, const float* sp, const float* wav, int B, int T, int L, float* wav_out,
                     void* stream) {
  if (!h || B <= 0 || T <= 0) return vfx_resunet_spec_1(h, sp, wav, B, T, L, wav_out, stream);
  const int64_t nb = h->cfg.n_fft / 2 + 1;
  return for_sub_batches(B, max_clips_per_launch(h, T, false, true, false), [&](int b, int n) {
    return vfx_resunet_spec_1(h, sp + (int64_t)b * T * nb, wav + (int64_t)b * L, n, T, L, wav_out + (int64_t)b * L, stream);
  });
}

int64_t vfx_vocoder_out_len(vfx_handle* h, int T) { return h ? vocoder_out_len(h->cfg, T) : -1; }

static int vfx_vocoder_1(vfx_handle* h, const float* mel_linear, int B, int T, float* wav_out, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(mel_linear && wav_out && B > 0 && T > 0, "bad argument");
  VFX_CHECK(h->voc, "vfx_vocoder: vocoder weights are not finalized");
  run_plan(h, key_of("vocoder", B, T), stream, {mel_linear, wav_out}, [&](PlanBuilder& pb) { build_vocoder(pb, B, T, ext(0), ext(1)); });
  VFX_API_END
}
int vfx_vocoder(vfx_handle* h, const float* mel_linear, int B, int T, float* wav_out, void* stream) {
  if (!h || B <= 0 || T <= 0) return vfx_vocoder_1(h, mel_linear, B, T, wav_out, stream);
  const int64_t Llong = vocoder_out_len(h->cfg, T);
  return for_sub_batches(B, max_clips_per_launch(h, T, false, false, true), [&](int b, int n) {
    return vfx_vocoder_1(h, mel_linear + (int64_t)b * T * 128, n, T, wav_out + (int64_t)b * Llong, stream);
  });
}

static int vfx_restore_gsr_1(vfx_handle* h, const float* wav, int B, int L, float* wav_out, float* logmel_out, int flags,
                             void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(wav && wav_out && B > 0, "bad argument");
  VFX_CHECK(L > h->cfg.n_fft / 2, "vfx_restore_gsr: clip too short for reflect padding (L=%d)", L);
  const int am = h->analysis_model;
  VFX_CHECK((am == VFX_MODEL_UNET_MEL ? (bool)h->unet[am] : (bool)h->analysis[am - VFX_MODEL_GRU_MEL]) && h->voc,
            "vfx_restore_gsr: weights are not finalized");
  const int T = frames_of(h, L);
  const int64_t Llong = vocoder_out_len(h->cfg, T);
  const int unify = flags & 1;
  // keyed on L, not on T: the plan's launches hold the sample count (STFT row stride and reflection point, trim_center) -- two
  // clips with the same frame count and different lengths must not share it (rounds 1-4 keyed on T: the second of two such
  // clips on one handle was framed and trimmed with the first one's length; found by the varlen comparison of round 5)
  run_plan(h, key_of("restore_gsr", B, L, unify + 2 * am), stream, {wav, wav_out, logmel_out}, [&](PlanBuilder& pb) {
    const int64_t nmel = (int64_t)B * T * 128;
    const size_t o_mel = pb.alloc_f(nmel), o_log = pb.alloc_f(nmel), o_den = pb.alloc_f(nmel);
    const size_t o_long = pb.alloc_f((int64_t)B * Llong), o_ws = pb.alloc_f(2 * B + 64), o_pk = pb.alloc_f(B + 64);
    vfx_handle* hh = pb.h;
    Plan* pl = pb.plan;
    // pre(): STFT -> magnitude -> mel (eval_gsr_voicefixer.py:19-25)
    pl->ops.push_back([=](const RunCtx& c) {
      launch_stft_mel(hh->fe, c.ext[0], B, L, T, reinterpret_cast<float*>(pl->bound_base + o_mel), nullptr, nullptr,
                      nullptr, 0, hh->cfg.hop, 1e-8f, c.stream);
    });
    if (am == VFX_MODEL_UNET_MEL) build_unet_mel(pb, B, T, arena_buf(o_mel), arena_buf(o_log));
    else build_analysis_mel(pb, am, B, T, arena_buf(o_mel), arena_buf(o_log));
    pl->ops.push_back([=](const RunCtx& c) {
      float* lg = reinterpret_cast<float*>(pl->bound_base + o_log);
      if (c.ext[2]) VFX_HIP(hipMemcpyAsync(c.ext[2], lg, sizeof(float) * nmel, hipMemcpyDeviceToDevice, c.stream));
      launch_from_log(lg, reinterpret_cast<float*>(pl->bound_base + o_mel), B, T, unify,
                      reinterpret_cast<float*>(pl->bound_base + o_ws), reinterpret_cast<float*>(pl->bound_base + o_den),
                      c.stream);
    });
    const BufRef peak_buf = arena_buf(o_pk);  // per-clip peak, produced by the vocoder tail
    build_vocoder(pb, B, T, arena_buf(o_den), arena_buf(o_long), &peak_buf);
    pl->ops.push_back([=](const RunCtx& c) {
      launch_peak_trim(reinterpret_cast<float*>(pl->bound_base + o_long), B, Llong, L,
                       reinterpret_cast<float*>(pl->bound_base + o_pk), c.ext[1], c.stream, c.flags);
    });
  });
  VFX_API_END
}
int vfx_restore_gsr(vfx_handle* h, const float* wav, int B, int L, float* wav_out, float* logmel_out, int flags,
                    void* stream) {
  if (!h || B <= 0 || L <= 0) return vfx_restore_gsr_1(h, wav, B, L, wav_out, logmel_out, flags, stream);
  const int T = L / h->cfg.hop + 1;
  return for_sub_batches(B, max_clips_per_launch(h, T, true, false, true), [&](int b, int n) {
    return vfx_restore_gsr_1(h, wav + (int64_t)b * L, n, L, wav_out + (int64_t)b * L,
                             logmel_out ? logmel_out + (int64_t)b * T * 128 : nullptr, flags, stream);
  });
}

// Clips of one ResUNet launch of a varlen call: a group's clip count is rounded up (dummy clips of zero frames) so that a test set
// meets a handful of (count, padded frames) shapes instead of one per group size -- a plan is 15 ms of host work to build
static int padded_group(int n) { return n <= 2 ? n : (n <= 8 ? (n + 1) / 2 * 2 : (n + 3) / 4 * 4); }

// A batch of clips of UNEQUAL length through the same per-segment body (the reference restores one file per call, of any
// length: evaluation_proc/eval.py:119-134, eval_gsr_voicefixer.py:47-74).  wav (B, Lmax): clip b = the first lengths[b] samples
// of row b.  Every clip gets what its own batch-of-one call computes:
//   * STFT: frames and the reflection at ITS end (fDomainHelper.py:26-28, center = True framing);
//   * ResUNet: all clips of a call share the padded frame count 64 * ceil(T_b / 64) -- a REQUIREMENT of this entry point (the
//     caller buckets by it) -- and a clip's rows past T_b are zeros like the network's own time padding (unet.py:75-77);
//   * vocoder: every launch stops the clip at its own length (zero padding, the k7 reflections, the tail of -4 frames);
//   * peak normalisation and trim_center per clip; wav_out (B, Lmax) and logmel_out (B, Tmax, 128) are zero past a clip's end.
//
// With a target (vfx_restore_gsr_varlen_scored, which has checked the lengths): target (B, Lmax), clip b = its first target_lengths[b]
// samples, metrics_out (B, VFX_N_HANDLER_METRICS) -- the handler's four mel scores (eval_gsr_voicefixer.py:56-64), scored where the
// log10 estimate and what the vocoder receives both exist.  Without one (all three NULL) the launches and the scratch are the same as ever.
//
// The first half -- pre() at the clips' own lengths, then the selected analysis module -- is varlen_analysis: vfx_restore_gsr_varlen goes
// on to the vocoder from it, vfx_validate_gsr_varlen to the log-mel L1 against the targets.  It places every tensor between the stages
// of the call in the handle's scratch (the vocoder's only when `vocoder`), `tail_bytes` more behind them for the caller's own, and
// leaves the log10 estimate in `lg`, copied to logmel_out (rows past a clip's last frame: zeros) when that is given.
struct VarlenAnalysis {
  int T = 0;
  std::vector<int> host;  // samples | frames | vocoder frames of the B clips
  struct Run { int b0, n, Tv; };
  std::vector<Run> runs;  // the vocoder's runs of consecutive clips (none without a vocoder)
  char* sc = nullptr;     // the scratch
  size_t o_den = 0, o_vmel = 0, o_long = 0, o_ws = 0, o_pk = 0, o_tail = 0;
  float *mel = nullptr, *lg = nullptr;
};
static size_t up_floats(int64_t n) { return (size_t)((n + 63) / 64 * 64) * sizeof(float); }

static void varlen_analysis(vfx_handle* h, const char* who, const float* wav, int B, int Lmax, const int* lengths, bool vocoder,
                            size_t tail_bytes, float* logmel_out, void* stream, VarlenAnalysis& va) {
  const int am = h->analysis_model;
  const int hop = h->cfg.hop;
  const int T = va.T = frames_of(h, Lmax);
  std::vector<int>& host = va.host;
  host.assign(3 * (size_t)B, 0);
  std::map<int, std::vector<int>, std::greater<int>> groups;  // padded frame count -> clips (longest group first)
  for (int b = 0; b < B; ++b) {
    const int Lb = lengths[b];
    VFX_CHECK(Lb > h->cfg.n_fft / 2 && Lb <= Lmax, "%s: clip %d has %d samples (need %d < length <= Lmax = %d)", who, b, Lb,
              h->cfg.n_fft / 2, Lmax);
    const int Tb = Lb / hop + 1;
    host[b] = Lb;
    host[B + b] = Tb;
    host[2 * (size_t)B + b] = Tb + Tb % 2 + 4;
    groups[(Tb + 63) / 64 * 64].push_back(b);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the per-clip lengths of THIS call (LensRow)
  constexpr int cap = kMaxVarlenClips;
  int* const d_l = h->lens_row(LENS_SAMPLES);
  int* const d_t = h->lens_row(LENS_FRAMES);
  int* const d_gt = h->lens_row(LENS_GROUP_FRAMES);
  int* const d_gi = h->lens_row(LENS_GROUP_INDEX);
  launch_set_lens(d_l, cap, host.data(), B, s);
  // ---- vocoder runs: consecutive clips (the callers hand them over sorted by length), each run on a compact (n, Tv, 128) tensor whose
  // frame count Tv is the run's own longest clip, rounded up to a multiple of 64 frames (a handful of plan shapes per test set)
  using Run = VarlenAnalysis::Run;
  std::vector<Run>& runs = va.runs;
  runs.clear();
  for (int b0 = 0; vocoder && b0 < B;) {
    int n = 0, tmax = 0;
    while (b0 + n < B) {
      const int tb = host[B + b0 + n];
      const int tnew = std::min(T, (std::max(tmax, tb) + 63) / 64 * 64);
      if (n > 0 && n + 1 > max_clips_per_launch(h, tnew, false, false, true)) break;
      // (measured, 128 clips of 2-8 s: cutting a run when its padding passes 7 % -- ~20 clips per run instead of ~43 -- changes
      // nothing: 0.777 -> 0.770 of an equal-length batch; what the mixed set loses is the ResUNet's deep levels on ~13 clips per group)
      tmax = tnew;
      ++n;
    }
    runs.push_back({b0, n, tmax});
    b0 += n;
  }
  // ---- the tensors between the stages (scratch): linear mel, log-mel estimate, restored linear mel of the batch; one ResUNet group's
  // compact input and output; one vocoder run's compact mel, long waveform, energy sums and peaks
  const int64_t nmel = (int64_t)B * T * 128;
  int64_t gmax = 0, vmel = 0, vlong = 0;
  int nmax = 0;
  for (auto& kv : groups) {
    if (am != VFX_MODEL_UNET_MEL) break;   // a GRU / DNN module runs on the batch tensors themselves
    const int step = std::max(1, max_clips_per_launch(h, kv.first, true, false, false) / 4 * 4);
    gmax = std::max<int64_t>(gmax, (int64_t)std::min(padded_group((int)kv.second.size()), step) * kv.first * 128);
  }
  for (auto& r : runs) {
    vmel = std::max<int64_t>(vmel, (int64_t)r.n * r.Tv * 128);
    vlong = std::max<int64_t>(vlong, (int64_t)r.n * vocoder_out_len(h->cfg, r.Tv));
    nmax = std::max(nmax, r.n);
  }
  auto up = up_floats;
  const size_t o_mel = 0, o_log = o_mel + up(nmel), o_den = o_log + up(nmel), o_gin = o_den + up(nmel), o_gout = o_gin + up(gmax),
               o_vmel = o_gout + up(gmax), o_long = o_vmel + up(vmel), o_ws = o_long + up(vlong), o_pk = o_ws + up(2 * B + 64),
               o_tail = o_pk + up(nmax + 64), o_end = o_tail + tail_bytes;  // (the tail: only a call with a target has one)
  // Handle-owned scratch beside the arena (grow-only): the tensors that travel BETWEEN the plans of one varlen call (every plan
  // places its own buffers from offset 0 of the arena).  Growing frees and re-allocates: the device is idle then (hipFree waits).
  char* const sc = h->scratch.ensure(h, o_end, 8, "the varlen scratch would have to grow from %zu to %zu bytes, but a hipGraph was captured "
                                     "from plan '%s': run the largest varlen batch once BEFORE capturing");
  float* const mel = reinterpret_cast<float*>(sc + o_mel);
  float* const lg = reinterpret_cast<float*>(sc + o_log);
  float* const gin = reinterpret_cast<float*>(sc + o_gin);
  float* const gout = reinterpret_cast<float*>(sc + o_gout);
  va.sc = sc;
  va.o_den = o_den, va.o_vmel = o_vmel, va.o_long = o_long, va.o_ws = o_ws, va.o_pk = o_pk, va.o_tail = o_tail;
  va.mel = mel;
  va.lg = lg;
  // ---- pre(): STFT -> magnitude -> mel, every clip framed and reflected at its own length (eval_gsr_voicefixer.py:19-25)
  launch_stft_mel(h->fe, wav, B, Lmax, T, mel, nullptr, nullptr, nullptr, 0, hop, 1e-8f, s, d_l);
  // ---- the mel ResUNet, one launch set per padded frame count (unet.py:75-77 pads every clip to ITS multiple of 64 frames): the
  // group's clips -- wherever they sit in the batch -- are gathered into a compact (Bg, Tpad, 128) tensor, restored, scattered back
  // ---- a GRU / DNN module: ONE run over the whole padded batch with the clips' own frame counts (row 1 of the table)
  if (am != VFX_MODEL_UNET_MEL) {
    run_plan(h, key_of(am == VFX_MODEL_GRU_MEL ? "gru_mel_vl" : "dnn_mel_vl", B, T), stream, {mel, lg}, [&](PlanBuilder& pb) {
      pb.lens_t = d_t;
      build_analysis_mel(pb, am, B, T, ext(0), ext(1));
    });
    groups.clear();
  }
  for (auto& kv : groups) {
    const int Tg = kv.first;
    const std::vector<int>& idx = kv.second;
    const int step = std::max(1, max_clips_per_launch(h, Tg, true, false, false) / 4 * 4);
    for (size_t at = 0; at < idx.size(); at += step) {
      const int n = (int)std::min<size_t>(step, idx.size() - at);
      const int np = std::min(padded_group(n), std::max(step, n));
      std::vector<int> hg(3 * (size_t)np, 0);
      for (int j = 0; j < np; ++j) {
        hg[j] = j < n ? host[B + idx[at + j]] : 0;                    // frames (a dummy clip: none -- all rows are padding)
        hg[(size_t)np + j] = idx[at + std::min(j, n - 1)];            // batch index
      }
      launch_set_lens(d_gt, cap, hg.data(), np, s);
      launch_gather_rows(mel, d_gi, gin, np, T, Tg, 128, s);
      run_plan(h, key_of("unet_mel_vg", np, Tg), stream, {gin, gout}, [&](PlanBuilder& pb) {
        pb.lens_t = d_gt;
        build_unet_mel(pb, np, Tg, ext(0), ext(1));
      });
      launch_scatter_rows(gout, d_gi, lg, n, T, Tg, 128, s);
    }
  }
  if (logmel_out) launch_copy_rows_masked(lg, logmel_out, B, T, 128, d_t, s);
}

// vfx_restore_gsr_varlen for at most kMaxVarlenClips clips; with a target, vfx_restore_gsr_varlen_scored
static int vfx_restore_gsr_varlen_1(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, float* wav_out,
                                    float* logmel_out, int flags, void* stream, const float* target = nullptr,
                                    const int* target_lengths = nullptr, double* metrics_out = nullptr) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(wav && wav_out && lengths && B > 0 && B <= kMaxVarlenClips, "bad argument");
  const int am = h->analysis_model;
  VFX_CHECK((am == VFX_MODEL_UNET_MEL ? (bool)h->unet[am] : (bool)h->analysis[am - VFX_MODEL_GRU_MEL]) && h->voc,
            "vfx_restore_gsr_varlen: weights are not finalized");
  const int hop = h->cfg.hop;
  const int T = frames_of(h, Lmax);
  const int64_t nmel = (int64_t)B * T * 128;
  VarlenAnalysis va;
  varlen_analysis(h, "vfx_restore_gsr_varlen", wav, B, Lmax, lengths, true, target ? up_floats(nmel) + handler_metrics_ws_bytes(B, T) : 0,
                  logmel_out, stream, va);
  hipStream_t s = static_cast<hipStream_t>(stream);
  constexpr int cap = kMaxVarlenClips;
  int* const d_t = h->lens_row(LENS_FRAMES);
  int* const d_gt = h->lens_row(LENS_GROUP_FRAMES);
  int* const d_gi = h->lens_row(LENS_GROUP_INDEX);
  int* const d_vl = h->lens_row(LENS_RUN_SAMPLES);
  int* const d_vt = h->lens_row(LENS_RUN_FRAMES);
  int* const d_vtp = h->lens_row(LENS_RUN_VOC_FRAMES);
  const int unify = flags & 1;
  const std::vector<int>& host = va.host;
  const std::vector<VarlenAnalysis::Run>& runs = va.runs;
  char* const sc = va.sc;
  float* const mel = va.mel;
  float* const lg = va.lg;
  float* const den = reinterpret_cast<float*>(sc + va.o_den);
  float* const vm = reinterpret_cast<float*>(sc + va.o_vmel);
  float* const wlong = reinterpret_cast<float*>(sc + va.o_long);
  float* const ws = reinterpret_cast<float*>(sc + va.o_ws);
  float* const pk = reinterpret_cast<float*>(sc + va.o_pk);
  launch_from_log(lg, mel, B, T, unify, ws, den, s, d_t);
  // ---- the handler's scores against the target: its mel by pre() at its own length, then the clip's four numbers over its own frames
  if (target) {
    const size_t o_tmel = va.o_tail, o_score = o_tmel + up_floats(nmel);
    int* const d_tl = h->lens_row(LENS_TARGET_SAMPLES);
    launch_set_frames(d_tl, target_lengths, B, s);
    float* const tmel = reinterpret_cast<float*>(sc + o_tmel);
    launch_stft_mel(h->fe, target, B, Lmax, T, tmel, nullptr, nullptr, nullptr, 0, hop, 1e-8f, s, d_tl);
    launch_handler_metrics(lg, den, tmel, B, T, d_t, sc + o_score, metrics_out, s);
  }
  // ---- the vocoder, one pass per run of clips: every launch stops a clip at its own length (round 5), so a run needs no common
  // padded frame count -- only the ResUNet does
  for (auto& r : runs) {
    std::vector<int> hv(3 * (size_t)r.n), hi(3 * (size_t)r.n, 0);
    for (int j = 0; j < r.n; ++j) {
      hv[j] = host[r.b0 + j];
      hv[(size_t)r.n + j] = host[B + r.b0 + j];
      hv[2 * (size_t)r.n + j] = host[2 * (size_t)B + r.b0 + j];
      hi[(size_t)r.n + j] = r.b0 + j;
    }
    launch_set_lens(d_vl, cap, hv.data(), r.n, s);
    launch_set_lens(d_gt, cap, hi.data(), r.n, s);      // (LENS_GROUP_INDEX = the run's batch indices for the gather)
    launch_gather_rows(den, d_gi, vm, r.n, T, r.Tv, 128, s);
    const int64_t Llong = vocoder_out_len(h->cfg, r.Tv);
    run_plan(h, key_of("voc_vl", r.n, r.Tv), stream, {vm, wlong, pk}, [&](PlanBuilder& pb) {
      pb.lens_t = d_vt;
      pb.lens_tp = d_vtp;
      const BufRef peak_buf = ext(2);
      build_vocoder(pb, r.n, r.Tv, ext(0), ext(1), &peak_buf);
    });
    launch_peak_trim_varlen(wlong, r.n, Llong, Lmax, hop, d_vl, d_vtp, pk, wav_out + (int64_t)r.b0 * Lmax, s, h->d_flags);
  }
  VFX_API_END
}
int vfx_restore_gsr_varlen(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, float* wav_out,
                           float* logmel_out, int flags, void* stream) {
  if (!h || B <= 0 || Lmax <= 0 || !lengths)
    return vfx_restore_gsr_varlen_1(h, wav, B, Lmax, lengths, wav_out, logmel_out, flags, stream);
  const int T = Lmax / h->cfg.hop + 1;
  // (the launches of one call are sub-batched inside it: the ResUNet per padded frame count, the vocoder per run of clips)
  return for_sub_batches(B, kMaxVarlenClips, [&](int b, int n) {
    return vfx_restore_gsr_varlen_1(h, wav + (int64_t)b * Lmax, n, Lmax, lengths + b, wav_out + (int64_t)b * Lmax,
                                    logmel_out ? logmel_out + (int64_t)b * T * 128 : nullptr, flags, stream);
  });
}

// What the two scored entries check of a whole batch before any sub-batch launches: the pointers, both lengths of every clip inside
// (n_fft/2, Lmax], at least 7 frames (skimage's 7 x 7 SSIM refuses a smaller image), and the reference's frame-count mismatch
// (eval_gsr_voicefixer.py:56-64 compares an estimate of lengths[b] / hop + 1 frames with a target of target_lengths[b] / hop + 1)
static int check_scored_batch(vfx_handle* h, const char* who, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                              const int* target_lengths, const float* wav_out, const double* metrics_out) {
  VFX_API_BEGIN
  VFX_CHECK(h != nullptr, "NULL handle");
  VFX_CHECK(wav && wav_out && lengths && B > 0 && Lmax > 0, "%s: bad argument", who);
  VFX_CHECK(target, "%s: target is NULL (a call without targets is the entry without _scored)", who);
  VFX_CHECK(metrics_out, "%s: metrics_out is NULL", who);
  VFX_CHECK(h->cfg.n_mels == 128, "%s: needs 128 mel bands", who);
  const int hop = h->cfg.hop, half = h->cfg.n_fft / 2;
  for (int b = 0; b < B; ++b) {
    const int Lb = lengths[b], Lt = target_lengths ? target_lengths[b] : Lb;
    VFX_CHECK(Lb > half && Lb <= Lmax, "%s: clip %d has %d samples (need %d < length <= Lmax = %d)", who, b, Lb, half, Lmax);
    VFX_CHECK(Lt > half && Lt <= Lmax, "%s: the target of clip %d has %d samples (need %d < length <= Lmax = %d)", who, b, Lt, half, Lmax);
    VFX_CHECK(Lb / hop + 1 >= 7, "%s: clip %d has %d samples, %d frames: the scores need at least 7 frames (%d samples)", who, b, Lb,
              Lb / hop + 1, 6 * hop);
    VFX_CHECK(Lt / hop == Lb / hop, "%s: clip %d has %d frames (%d samples) but its target has %d (%d samples)", who, b, Lb / hop + 1, Lb,
              Lt / hop + 1, Lt);
  }
  VFX_API_END
}

int vfx_restore_gsr_varlen_scored(vfx_handle* h, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                                  const int* target_lengths, float* wav_out, float* logmel_out, double* metrics_out, int flags,
                                  void* stream) {
  if (const int rc = check_scored_batch(h, "vfx_restore_gsr_varlen_scored", wav, target, B, Lmax, lengths, target_lengths, wav_out, metrics_out))
    return rc;
  if (!target_lengths) target_lengths = lengths;
  const int T = Lmax / h->cfg.hop + 1;
  return for_sub_batches(B, kMaxVarlenClips, [&](int b, int n) {
    return vfx_restore_gsr_varlen_1(h, wav + (int64_t)b * Lmax, n, Lmax, lengths + b, wav_out + (int64_t)b * Lmax,
                                    logmel_out ? logmel_out + (int64_t)b * T * 128 : nullptr, flags, stream, target + (int64_t)b * Lmax,
                                    target_lengths + b, metrics_out + (int64_t)b * VFX_N_HANDLER_METRICS);
  });
}

// val_l of models/gsr_voicefixer.py:264-277 per clip: the first half of vfx_restore_gsr_varlen (varlen_analysis), then to_log(mel(target))
// at the target's own length and the L1 over the clip's own T_b x 128 values.  No vocoder runs and none has to be loaded.
static int vfx_validate_gsr_varlen_1(vfx_handle* h, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                                     const int* target_lengths, float* logmel_out, double* val_l, void* stream) {
  VFX_API_BEGIN_HS(h, stream)
  const int am = h->analysis_model;
  VFX_CHECK(am == VFX_MODEL_UNET_MEL ? (bool)h->unet[am] : (bool)h->analysis[am - VFX_MODEL_GRU_MEL],
            "vfx_validate_gsr_varlen: weights of the analysis module are not finalized");
  const int hop = h->cfg.hop;
  const int T = frames_of(h, Lmax);
  const int64_t nmel = (int64_t)B * T * 128;
  const int nchunk = l1_chunks((int64_t)T * 128);
  VarlenAnalysis va;
  varlen_analysis(h, "vfx_validate_gsr_varlen", wav, B, Lmax, lengths, false, up_floats(nmel) + (size_t)B * nchunk * sizeof(double), logmel_out,
                  stream, va);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* const tlog = reinterpret_cast<float*>(va.sc + va.o_tail);
  double* const chunk_ws = reinterpret_cast<double*>(va.sc + va.o_tail + up_floats(nmel));
  int* const d_tl = h->lens_row(LENS_TARGET_SAMPLES);
  int* const d_n = h->lens_row(LENS_LOSS_COUNT);
  std::vector<int> count(B);
  for (int b = 0; b < B; ++b) count[b] = 128 * va.host[(size_t)B + b];  // the first T_b rows of a clip are contiguous
  launch_set_frames(d_tl, target_lengths, B, s);
  launch_set_frames(d_n, count.data(), B, s);
  launch_stft_mel(h->fe, target, B, Lmax, T, tlog, nullptr, nullptr, nullptr, 1, hop, 1e-8f, s, d_tl);
  launch_l1_rows(va.lg, tlog, B, (int64_t)T * 128, d_n, nchunk, chunk_ws, s);
  launch_loss_final(chunk_ws, nchunk, d_n, nullptr, 0, nullptr, 0, 0, val_l, 1, B, s);
  VFX_API_END
}

// What vfx_validate_gsr_varlen checks of a whole batch before any sub-batch launches: check_scored_batch's rules without the 7-frame
// minimum (no SSIM is computed here)
static int check_validate_batch(vfx_handle* h, const char* who, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                                const int* target_lengths, const double* val_l) {
  VFX_API_BEGIN
  VFX_CHECK(h != nullptr, "NULL handle");
  VFX_CHECK(wav && lengths && B > 0 && Lmax > 0, "%s: bad argument", who);
  VFX_CHECK(target, "%s: target is NULL", who);
  VFX_CHECK(val_l, "%s: val_l is NULL", who);
  VFX_CHECK(h->cfg.n_mels == 128, "%s: needs 128 mel bands", who);
  const int hop = h->cfg.hop, half = h->cfg.n_fft / 2;
  for (int b = 0; b < B; ++b) {
    const int Lb = lengths[b], Lt = target_lengths ? target_lengths[b] : Lb;
    VFX_CHECK(Lb > half && Lb <= Lmax, "%s: clip %d has %d samples (need %d < length <= Lmax = %d)", who, b, Lb, half, Lmax);
    VFX_CHECK(Lt > half && Lt <= Lmax, "%s: the target of clip %d has %d samples (need %d < length <= Lmax = %d)", who, b, Lt, half, Lmax);
    VFX_CHECK(Lt / hop == Lb / hop, "%s: clip %d has %d frames (%d samples) but its target has %d (%d samples)", who, b, Lb / hop + 1, Lb,
              Lt / hop + 1, Lt);
  }
  VFX_API_END
}

int vfx_validate_gsr_varlen(vfx_handle* h, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                            const int* target_lengths, float* logmel_out, double* val_l, void* stream) {
  if (const int rc = check_validate_batch(h, "vfx_validate_gsr_varlen", wav, target, B, Lmax, lengths, target_lengths, val_l)) return rc;
  if (!target_lengths) target_lengths = lengths;
  const int T = Lmax / h->cfg.hop + 1;
  return for_sub_batches(B, kLossMaxClips, [&](int b, int n) {
    return vfx_validate_gsr_varlen_1(h, wav + (int64_t)b * Lmax, target + (int64_t)b * Lmax, n, Lmax, lengths + b, target_lengths + b,
                                     logmel_out ? logmel_out + (int64_t)b * T * 128 : nullptr, val_l + b, stream);
  });
}

// The spectrogram-domain twin: the per-segment body of handler_ssr_unet (eval_ssr_unet.py:77-114: sp = |STFT(wav)|, model(sp, wav))
// for a batch of clips of unequal length -- per clip the frames and reflection of its own length, the trunk's zero time padding
// behind its own last frame (unet_v2.py:103-110), the ISTFT to its own length (fDomainHelper.py:30-32); zeros past its end.
// Same requirement as vfx_restore_gsr_varlen: one padded frame count per call.
// With a target (vfx_restore_ssr_varlen_scored): the four scores of eval_ssr_unet.py:116-126 on the mel of the restored clip and of its target
static int vfx_restore_ssr_varlen_1(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, float* wav_out, void* stream,
                                    const float* target = nullptr, const int* target_lengths = nullptr, double* metrics_out = nullptr) {
  VFX_API_BEGIN_HS(h, stream)
  VFX_CHECK(wav && wav_out && lengths && B > 0 && B <= kMaxVarlenClips, "bad argument");
  VFX_CHECK(h->unet[VFX_MODEL_UNET_SPEC], "vfx_restore_ssr_varlen: weights of the spectrogram ResUNet are not finalized");
  const int hop = h->cfg.hop;
  const int T = frames_of(h, Lmax), Tpad = (T + 63) / 64 * 64;
  std::vector<int> host(3 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    const int Lb = lengths[b];
    VFX_CHECK(Lb > h->cfg.n_fft / 2 && Lb <= Lmax, "vfx_restore_ssr_varlen: clip %d has %d samples (need %d < length <= Lmax = %d)", b, Lb,
              h->cfg.n_fft / 2, Lmax);
    const int Tb = Lb / hop + 1;
    VFX_CHECK((Tb + 63) / 64 * 64 == Tpad, "vfx_restore_ssr_varlen: clip %d has %d frames (padded %d) but the batch's longest row pads to %d -- "
              "the clips of one call must share 64 * ceil(T / 64): bucket them by it", b, Tb, (Tb + 63) / 64 * 64, Tpad);
    host[b] = Lb;
    host[B + b] = Tb;
    host[2 * (size_t)B + b] = Tb;  // (no vocoder here)
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* const d_l = h->lens_row(LENS_SAMPLES);
  int* const d_t = h->lens_row(LENS_FRAMES);
  launch_set_lens(d_l, kMaxVarlenClips, host.data(), B, s);
  const size_t nsp = (size_t)B * T * (h->cfg.n_fft / 2 + 1);
  auto plan = run_plan(h, key_of("restore_ssr_vl", B, Lmax), stream, {wav}, [&](PlanBuilder& pb) {
    auto& nm = pb.plan->named;
    const size_t o_sp = pb.alloc_f(nsp), o_cos = pb.alloc_f(nsp), o_sin = pb.alloc_f(nsp), o_re = pb.alloc_f(nsp), o_im = pb.alloc_f(nsp);
    nm["re"] = o_re;
    nm["im"] = o_im;
    vfx_handle* hh = pb.h;
    Plan* pl = pb.plan;
    pb.lens_t = d_t;
    pl->ops.push_back([=](const RunCtx& c) {  // one STFT for magnitude and phase (the reference runs two: eval_ssr_unet.py:80, unet_v2.py:96)
      launch_stft_mel(hh->fe, c.ext[0], B, Lmax, T, nullptr, reinterpret_cast<float*>(pl->bound_base + o_sp),
                      reinterpret_cast<float*>(pl->bound_base + o_cos), reinterpret_cast<float*>(pl->bound_base + o_sin), 0, hh->cfg.hop,
                      1e-8f, c.stream, d_l);
    });
    build_unet_spec(pb, B, T, arena_buf(o_sp), arena_buf(o_cos), arena_buf(o_sin), arena_buf(o_re), arena_buf(o_im));
  });
  launch_istft(h->fe, reinterpret_cast<float*>(h->arena.p + plan->named["re"]), reinterpret_cast<float*>(h->arena.p + plan->named["im"]), B, T,
               Lmax, hop, wav_out, s, d_l);
  if (target) {  // mel_out = mel(|STFT(out)|), target_mel = pre(target), both clamped at 1e-8 and framed at the clip's own length
    const size_t nmel = ((size_t)B * T * 128 * sizeof(float) + 255) / 256 * 256;
    char* const sc = h->scratch.ensure(h, 2 * nmel + handler_metrics_ws_bytes(B, T), 8, "the varlen scratch would have to grow from %zu to %zu "
                                       "bytes, but a hipGraph was captured from plan '%s': run the largest scored batch once BEFORE capturing");
    float* const emel = reinterpret_cast<float*>(sc);
    float* const tmel = reinterpret_cast<float*>(sc + nmel);
    int* const d_tl = h->lens_row(LENS_TARGET_SAMPLES);
    launch_set_frames(d_tl, target_lengths, B, s);
    launch_stft_mel(h->fe, wav_out, B, Lmax, T, emel, nullptr, nullptr, nullptr, 0, hop, 1e-8f, s, d_l);
    launch_stft_mel(h->fe, target, B, Lmax, T, tmel, nullptr, nullptr, nullptr, 0, hop, 1e-8f, s, d_tl);
    launch_mel_metrics(emel, tmel, B, T, d_t, sc + 2 * nmel, metrics_out, s);
  }
  VFX_API_END
}
int vfx_restore_ssr_varlen(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, float* wav_out, void* stream) {
  if (!h || B <= 0 || Lmax <= 0 || !lengths) return vfx_restore_ssr_varlen_1(h, wav, B, Lmax, lengths, wav_out, stream);
  const int T = Lmax / h->cfg.hop + 1;
  return for_sub_batches(B, std::min(kMaxVarlenClips, max_clips_per_launch(h, T, false, true, false)), [&](int b, int n) {
    return vfx_restore_ssr_varlen_1(h, wav + (int64_t)b * Lmax, n, Lmax, lengths + b, wav_out + (int64_t)b * Lmax, stream);
  });
}

int vfx_restore_ssr_varlen_scored(vfx_handle* h, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                                  const int* target_lengths, float* wav_out, double* metrics_out, void* stream) {
  if (const int rc = check_scored_batch(h, "vfx_restore_ssr_varlen_scored", wav, target, B, Lmax, lengths, target_lengths, wav_out, metrics_out))
    return rc;
  if (!target_lengths) target_lengths = lengths;
  const int T = Lmax / h->cfg.hop + 1;
  return for_sub_batches(B, std::min(kMaxVarlenClips, max_clips_per_launch(h, T, false, true, false)), [&](int b, int n) {
    return vfx_restore_ssr_varlen_1(h, wav + (int64_t)b * Lmax, n, Lmax, lengths + b, wav_out + (int64_t)b * Lmax, stream,
                                    target + (int64_t)b * Lmax, target_lengths + b, metrics_out + (int64_t)b * VFX_N_HANDLER_METRICS);
  });
}

// ---------------------------------------------------------------------------------------------
// streaming sessions: the bookkeeping is stream_sched.cpp's, the kernels stream.hip's; here the two meet the device memory
// ---------------------------------------------------------------------------------------------
}  // extern "C"

struct vfx_stream {
  vfx_handle* h = nullptr;
  vfx::StreamSched sched;
  int mode, win, par;
  int cap_in, cap_out;
  float scale;
  float *d_in = nullptr, *d_acc = nullptr, *d_out = nullptr, *d_window = nullptr;
  int row_len = 0;   // of the outstanding group
  std::vector<vfx::StreamCopyRow> copy_rows;
  std::vector<vfx::StreamGatherRow> gather_rows;
  std::vector<vfx::StreamOlaRow> ola_rows;
  std::vector<vfx::StreamBoxRow> box_rows;
  vfx_stream(vfx_handle* h_, int slots, int mode_, int win_, int par_, float scale_, int64_t ci, int64_t co)
      : h(h_), sched(slots, mode_, win_, par_, ci, co), mode(mode_), win(win_), par(par_), cap_in((int)ci), cap_out((int)co), scale(scale_) {}
  ~vfx_stream() {
    (void)hipFree(d_in);
    (void)hipFree(d_acc);
    (void)hipFree(d_out);
    (void)hipFree(d_window);
  }
};

// the session's handle names the device and the turn: a NULL session is refused before it is looked into
#define VFX_STREAM_BEGIN(st, stream)              \
  if (!(st)) {                                    \
    ::vfx::set_error("vfx_stream: NULL session"); \
    return 1;                                     \
  }                                               \
  VFX_API_BEGIN_HS((st)->h, stream)
#define VFX_SCHED(call) VFX_CHECK((call), "vfx_stream: %s", st->sched.error.c_str())

extern "C" {

int vfx_stream_create(vfx_handle* h, int slots, int mode, int win, int hop_or_margin, const float* window, float scale, int64_t capacity,
                      int64_t out_capacity, vfx_stream** out) {
  VFX_API_BEGIN_H(h)
  VFX_CHECK(out != nullptr, "vfx_stream_create: st is NULL");
  std::string why;
  VFX_CHECK(StreamSched::check_geometry(slots, mode, win, hop_or_margin, capacity, out_capacity, &why), "vfx_stream_create: %s", why.c_str());
  auto st = std::make_unique<vfx_stream>(h, slots, mode, win, hop_or_margin, scale, capacity, out_capacity);
  VFX_HIP(hipMalloc(&st->d_in, (size_t)slots * capacity * sizeof(float)));
  VFX_HIP(hipMalloc(&st->d_out, (size_t)slots * out_capacity * sizeof(float)));
  if (mode == STREAM_OLA) {
    VFX_HIP(hipMalloc(&st->d_acc, (size_t)slots * 2 * win * sizeof(float)));
    VFX_HIP(hipMemset(st->d_acc, 0, (size_t)slots * 2 * win * sizeof(float)));
  }
  if (window) {
    VFX_HIP(hipDeviceSynchronize());   // the caller's window may still be on its way on some stream
    VFX_HIP(hipMalloc(&st->d_window, (size_t)win * sizeof(float)));
    VFX_HIP(hipMemcpy(st->d_window, window, (size_t)win * sizeof(float), hipMemcpyDeviceToDevice));
  }
  VFX_HIP(hipDeviceSynchronize());
  *out = st.release();
  VFX_API_END
}

int vfx_stream_destroy(vfx_stream* st) {
  if (!st) return 0;
  VFX_API_BEGIN_H(st->h)
  VFX_HIP(hipDeviceSynchronize());
  delete st;
  VFX_API_END
}

int vfx_stream_open(vfx_stream* st, int* slot) {
  VFX_API_BEGIN
  VFX_CHECK(st && slot, "vfx_stream_open: NULL argument");
  VFX_SCHED(st->sched.open(slot));
  VFX_API_END
}

int vfx_stream_close(vfx_stream* st, int slot) {
  VFX_API_BEGIN
  VFX_CHECK(st != nullptr, "vfx_stream_close: NULL session");
  VFX_SCHED(st->sched.close(slot));
  VFX_API_END
}

int vfx_stream_available(vfx_stream* st, int slot, int64_t* n) {
  VFX_API_BEGIN
  VFX_CHECK(st && n, "vfx_stream_available: NULL argument");
  VFX_CHECK(st->sched.available(slot, n), "vfx_stream_available: slot %d does not exist", slot);
  VFX_API_END
}

int vfx_stream_room(vfx_stream* st, int slot, int64_t* n) {
  VFX_API_BEGIN
  VFX_CHECK(st && n, "vfx_stream_room: NULL argument");
  VFX_CHECK(st->sched.room(slot, n), "vfx_stream_room: slot %d does not exist", slot);
  VFX_API_END
}

int vfx_stream_state(vfx_stream* st, int slot, int64_t* fed, int64_t* released) {
  VFX_API_BEGIN
  VFX_CHECK(st && fed && released, "vfx_stream_state: NULL argument");
  VFX_CHECK(st->sched.state(slot, fed, released), "vfx_stream_state: slot %d does not exist", slot);
  VFX_API_END
}

int vfx_stream_push(vfx_stream* st, int n, const int* slots, const int64_t* counts, const float* packed_blocks, void* stream) {
  VFX_STREAM_BEGIN(st, stream)
  VFX_CHECK(n >= 0 && (n == 0 || (slots && counts)), "vfx_stream_push: bad argument");
  for (int i = 0; i < n; ++i) VFX_CHECK(counts[i] <= 0 || packed_blocks, "vfx_stream_push: packed_blocks is NULL");
  VFX_SCHED(st->sched.push(n, slots, counts, &st->copy_rows));   // refused before anything is copied
  launch_stream_copy(true, st->d_in, st->cap_in, const_cast<float*>(packed_blocks), st->copy_rows, static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_stream_next(vfx_stream* st, int max_rows, float* chunks_out, int* rows, int* row_len, void* stream) {
  VFX_STREAM_BEGIN(st, stream)
  VFX_CHECK(chunks_out && rows && row_len, "vfx_stream_next: NULL argument");
  VFX_SCHED(st->sched.next(max_rows, &st->gather_rows, &st->row_len));
  *rows = (int)st->gather_rows.size();
  *row_len = st->row_len;
  if (*rows) launch_stream_gather(st->d_in, st->cap_in, st->row_len, chunks_out, st->gather_rows, static_cast<hipStream_t>(stream));
  VFX_API_END
}

int vfx_stream_put(vfx_stream* st, const float* frames, void* stream) {
  VFX_STREAM_BEGIN(st, stream)
  VFX_CHECK(frames != nullptr, "vfx_stream_put: frames is NULL");
  VFX_SCHED(st->sched.put(&st->ola_rows, &st->box_rows));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (st->mode == STREAM_OLA)
    launch_stream_ola(frames, st->d_window, st->scale, st->win, st->par, st->d_acc, st->d_out, st->cap_out, st->ola_rows, s);
  else
    launch_stream_box(frames, st->row_len, st->d_window, st->scale, st->d_out, st->cap_out, st->box_rows, s);
  VFX_API_END
}

int vfx_stream_pop(vfx_stream* st, int n, const int* slots, const int64_t* max_counts, float* packed_out, int64_t* counts_out,
                   void* stream) {
  VFX_STREAM_BEGIN(st, stream)
  VFX_CHECK(n >= 0 && (n == 0 || (slots && max_counts && counts_out)), "vfx_stream_pop: bad argument");
  if (!packed_out) {   // nothing may be taken without a place to put it
    for (int i = 0; i < n; ++i) {
      int64_t have = 0;
      VFX_CHECK(st->sched.available(slots[i], &have), "vfx_stream_pop: slot %d does not exist", slots[i]);
      VFX_CHECK(have == 0 || max_counts[i] == 0, "vfx_stream_pop: packed_out is NULL");
    }
  }
  VFX_SCHED(st->sched.pop(n, slots, max_counts, &st->copy_rows, counts_out));
  launch_stream_copy(false, st->d_out, st->cap_out, packed_out, st->copy_rows, static_cast<hipStream_t>(stream));
  VFX_API_END
}

// ---------------------------------------------------------------------------------------------
// live kernel timing (bench.py roofline): HIP events around every tap-convolution launch, on the
// stream the kernels are launched on.
// ---------------------------------------------------------------------------------------------
int vfx_profile_begin(vfx_handle* h) {
  VFX_API_BEGIN_H(h)
  h->prof.enabled = true;
  h->prof.launches.clear();
  VFX_API_END
}

// Synchronises, then returns: number of launches, sum of their durations (ms) and of their
// algorithmic FLOPs (2 * M * Cout * K).  Any out pointer may be NULL.
int vfx_profile_end(vfx_handle* h, int64_t* launches, double* total_ms, double* total_flops) {
  VFX_API_BEGIN_H(h)
  VFX_HIP(hipDeviceSynchronize());
  double ms = 0, fl = 0;
  FILE* dump = nullptr;
  if (const char* path = getenv("VFX_PROFILE_DUMP")) dump = fopen(path, "w");
  if (dump) fprintf(dump, "idx,kernel,M,Cout,K,nseg,ntaps0,C0,Wi,sw,ms,tflops,bytes,design_bytes\n");
  for (size_t i = 0; i < h->prof.launches.size(); ++i) {
    const LaunchRecord& r = h->prof.launches[i];
    float t = 0.f;
    VFX_HIP(hipEventElapsedTime(&t, r.begin, r.end));
    if (dump)
      fprintf(dump, "%zu,%s,%d,%d,%d,%d,%d,%d,%d,%d,%.4f,%.2f,%.0f,%.0f\n", i, r.kernel, r.M, r.Cout, r.K, r.nseg, r.ntaps0, r.C0, r.Wi,
              r.sw, t, r.flops / (t * 1e-3) / 1e12, r.bytes, r.design_bytes);
    ms += t;
    fl += r.flops;
    (void)hipEventDestroy(r.begin);
    (void)hipEventDestroy(r.end);
  }
  if (dump) fclose(dump);
  if (launches) *launches = (int64_t)h->prof.launches.size();
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  h->prof.launches.clear();
  h->prof.enabled = false;
  VFX_API_END
}

}  // extern "C"
