/*
 * vfx.h -- C ABI of libvfx.so: MI355X-native (gfx950) VoiceFixer 44.1 kHz inference hot path.
 *
 * Drop-in boundary for the reference haoheliu/voicefixer_main.  The reference is pure
 * Python/PyTorch and has no FFI of its own; each entry point below replaces the arithmetic
 * of one reference call (file:line cited) and is what a ctypes binding inside the
 * reference's own modules would bind.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers to contiguous fp32 unless stated otherwise;
 *     the caller (PyTorch) owns inputs and outputs, the library never frees them;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it, no entry point synchronises the device except
 *     vfx_create / vfx_load_tensor / vfx_finalize_weights / vfx_reserve / vfx_take_flags;
 *   - the handle owns a copy of the weights and one workspace arena; it is NOT thread-safe;
 *   - calls on DIFFERENT streams of one device (two handles, or one handle moved between streams) take turns on the GPU
 *     timeline: the library does not let its own launches of two streams overlap (profiles/r05_two_streams.md); a call made
 *     while its stream is being captured into a hipGraph is exempt -- bracket the graph's replays with vfx_turn_begin /
 *     vfx_turn_end when another stream of the device may run calls of this library at the same time;
 *   - every function returns 0 on success, non-zero on failure; vfx_last_error() then
 *     returns a human-readable message (thread-local).
 *   - T = L / hop + 1 frames (center=True framing); Tpad = 64*ceil(T/64).
 */
#ifndef VFX_H_
#define VFX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfx_handle vfx_handle;

#define VFX_MAX_STAGES 8

/* model ids for weights / plans */
enum { VFX_MODEL_UNET_MEL = 0, VFX_MODEL_UNET_SPEC = 1, VFX_MODEL_VOCODER = 2,
       VFX_MODEL_FRONTEND = 3, /* buffers of f_helper / mel: "mel.fb" (1025,128) */
       VFX_MODEL_GRU_MEL = 4,  /* the bi_gru analysis module of Generator (gsr_voicefixer.py:59-68) */
       VFX_MODEL_DNN_MEL = 5   /* the dnn analysis module (gsr_voicefixer.py:69-87) */ };

/* sticky device-side flags returned by vfx_take_flags */
enum {
  VFX_FLAG_NEGATIVE_INPUT = 1, /* to_log saw a negative value (pytorch_util.py:158) */
  VFX_FLAG_F16_SATURATED = 2,  /* precision 2: an activation of the vocoder left the fp16 range (|x| > 65504, or was
                                  not a number) and was clamped -- the result of that call is not trustworthy; re-run
                                  it with precision 1 */
  VFX_FLAG_PEAK_NORMALISED = 4 /* vfx_restore_gsr divided a clip by its peak (> 1): the reference prints "Warning:
                                  Exceed energy limit" there (eval_gsr_voicefixer.py:68-70); informational */
};

/* vfx_config.tuning: kernel-selection switches for A/B measurements and bisecting (0 = the shipped configuration; every
 * bit selects an older / simpler form of the same arithmetic, results stay within the mode's tolerances).  Read when a
 * plan is built; vfx_create reports a non-zero mask on stderr.  Every bit is exercised by the GPU test suite. */
enum {
  VFX_TUNE_NO_FUSED_STACKS = 1,    /* vocoder ResStack layers (C = 64, 128) as two tap-convolution launches per layer */
  VFX_TUNE_NO_FUSED_WIDE = 2,      /* ... the C = 256 layers of the 16-bit mode as two launches per layer (two-form trunk) */
  VFX_TUNE_NO_FUSED_UNET = 4,      /* ConvBlockRes of the ResUNets as two launches each (fused: the identity-shortcut blocks at
                                      C = 32, 64, the entry block and the two-source block of the full-resolution level) */
  VFX_TUNE_NO_PERSISTENT_C64 = 8,  /* 16-bit mode, C = 64 layers on k_resblock instead of the persistent kernel */
  VFX_TUNE_NO_PAIRS = 16,          /* 16-bit mode, C = 64 / 128: one launch per layer (no layer pairs) */
  VFX_TUNE_NO_SPLITK = 32,         /* no split-K in the deep ResUNet levels */
  VFX_TUNE_F32_TRUNK = 64,         /* 16-bit mode: the residual trunk of the fused ResStacks (C = 64 / 128 / 256) travels as fp32
                                      between the layers (the round-3 form: 8 - 12 bytes per element and layer) instead of
                                      fp16 (4 bytes per element and layer; the sums themselves are fp32 in registers either way) */
  VFX_TUNE_SMALL_2D_TILES = 128,   /* fused ConvBlockRes of the ResUNets at C = 32: 8 x 16 / 16 x 8 h tiles (84 outputs per 128 positions)
                                      instead of 16 x 16 (196 per 256); the entry block (Cin = 1) and the two-source block of that
                                      level, which exist on 16 x 16 tiles only, as two launches each */
  VFX_TUNE_NO_FUSED_UPSAMPLERS = 512, /* 16-bit mode: the vocoder's ConvTranspose1d upsamplers as phased tap-convolution launches (one block per
                                      tile, phase and cout range) instead of k_up16 (one block per tile of input positions, all phases) */
  VFX_TUNE_OLD_BLOCK2D = 1024,     /* the identity ConvBlockRes of ResUNet level 1 (C = 32, 16 x 16 tiles) on k_resblock (one tile per block, LDS-DMA
                                      patch, swizzled rows) instead of the persistent k_block2d32 (round 6) */
  VFX_TUNE_TWO_LAUNCH_UPSAMPLERS = 2048, /* the mel ResUNet's 2 x upsamplers (odd output width) as two launches of two column phases each (one
                                      per output row class: the round-4 form) instead of one launch of four phases (round 6) */
  VFX_TUNE_DEBUG_POISON_ARENA = 256 /* debug aid, no kernel selection: the handle's workspace arena is filled with NaN patterns when
                                      it grows and before every call, so that a kernel reading a buffer nobody wrote shows up */
};

typedef struct vfx_config {
  /* front-end: config/vctk_base_voicefixer_unet.json:68-78 */
  int sample_rate;  /* 44100 */
  int n_fft;        /* 2048 (only value supported by the FFT kernels) */
  int hop;          /* 441 */
  int n_mels;       /* 128 */
  /* TFGAN vocoder layer table (third-party `voicefixer` package; see oracle/vocoder.py) */
  int voc_cond_channels;              /* 512 */
  int voc_cond_layers;                /* 5 */
  int voc_channels;                   /* 1024 */
  int voc_n_stages;                   /* 4 */
  int voc_scales[VFX_MAX_STAGES];     /* 7,7,3,3 */
  int voc_depth[VFX_MAX_STAGES];      /* 8,8,8,8 */
  int voc_dilation_base;              /* 3 */
  float voc_min_db;                   /* -115 */
  float voc_amp_floor;                /* 1e-5 */
  float voc_norm_range;               /* 4 */
  float voc_up_slope;                 /* 0.2 */
  float voc_res_slope;                /* 0.01 */
  /* arithmetic of the GEMM-shaped layers:
   * 1 (default) = split-bf16: every operand is hi + lo (two bf16), products hi*hi + hi*lo +
   *     lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (~2^-16 relative operand
   *     error; log-mel L1 vs the fp64 oracle 4e-5..8e-5, bar 1e-3);
   * 0 = exact fp32 (v_mfma_f32_32x32x2_f32), log-mel L1 5e-6..1e-5, ~1.8x slower;
   * 2 = "16-bit vocoder": the ResUNets as 1 (they carry the log-mel bar), the TFGAN vocoder on
   *     fp16 operands (the hi halves of the same layouts hold fp16 values and are the only ones
   *     loaded and multiplied: one v_mfma_f32_32x32x16_f16 per product, fp32 accumulation,
   *     saturating conversion).  BASELINE.json's 16-bit operand mode for config 2; fp16 rather
   *     than bf16 because bf16 operands hold the waveform to 40 dB SI-SDR only. */
  int precision;
  int tuning;  /* mask of VFX_TUNE_*; 0 = default */
} vfx_config;

/* Fill *cfg with the reference's hyper-parameters. */
int vfx_default_config(vfx_config* cfg);

/* Create / destroy a handle bound to HIP device `device`. */
int vfx_create(int device, const vfx_config* cfg, vfx_handle** out);
int vfx_destroy(vfx_handle* h);
const char* vfx_last_error(void);

/*
 * Weights.  `name` is the reference state_dict key (models/components/unet.py:22-53,
 * modules.py:223-261) for the UNet models, or the vocoder key convention documented in
 * oracle/vocoder.py.  `data` is a HOST pointer to contiguous fp32 of the given shape
 * (PyTorch layout).  Replaces `load_from_checkpoint` + `model.to(device)`
 * (eval_gsr_voicefixer.py:33-40).  vfx_finalize_weights folds eval-mode BatchNorm into
 * per-channel affine pairs, re-packs conv weights into the kernels' K-chunked layout and
 * uploads them.
 */
int vfx_load_tensor(vfx_handle* h, int model, const char* name, const float* data,
                    const int64_t* shape, int ndim);
int vfx_finalize_weights(vfx_handle* h, int model);

/* Workspace (bytes) a call of `model` needs for batch B and T frames; vfx_reserve grows the
 * arena up-front so that later calls never allocate (required before graph capture). */
size_t vfx_workspace_bytes(vfx_handle* h, int model, int B, int T);
int vfx_reserve(vfx_handle* h, int model, int B, int T);
/* A call made while its stream is being captured into a hipGraph pins its plan: the graph's kernel nodes hold the plan's device
 * parameter blocks and absolute pointers into the workspace arena, so from then on the handle refuses to grow (= move) its arena
 * -- a larger call returns an error instead of freeing memory the graph replays into.  vfx_unpin_plans declares that every graph
 * captured from this handle has been destroyed: plans become evictable again and the arena may grow. */
int vfx_unpin_plans(vfx_handle* h);

/*
 * STFT front-end: FDomainHelper.wav_to_spectrogram_phase (tools/pytorch/modules/
 * fDomainHelper.py:60-89) fused with MelScale.forward (tools/pytorch/mel_scale.py:52-64) and
 * optionally to_log (tools/pytorch/pytorch_util.py:157-159).
 *   wav (B, L) -> any non-NULL of: sp, cosp, sinp (B, T, 1025) ; mel (B, T, 128).
 * log10_mel != 0 writes log10(max(mel, 1e-8)) instead of linear mel.
 */
int vfx_stft_mel(vfx_handle* h, const float* wav, int B, int L, float* mel, float* sp,
                 float* cosp, float* sinp, int log10_mel, void* stream);

/* FDomainHelper.spectrogram_phase(input, eps) (tools/pytorch/modules/fDomainHelper.py:60-65) with the caller's eps:
 * mag = sqrt(clamp(re^2 + im^2, eps, inf)), cos = re / mag, sin = im / mag; any of sp / cosp / sinp (B, T, 1025) may be
 * NULL.  eps = 0 (the reference default of this method) gives 0/0 = NaN phases at exactly silent bins, as the
 * reference does; vfx_stft_mel is the eps = 1e-8 case every handler call site uses (fDomainHelper.py:67). */
int vfx_stft_phase(vfx_handle* h, const float* wav, int B, int L, float* sp, float* cosp, float* sinp,
                   float eps, void* stream);

/* MelScale.forward alone (tools/pytorch/mel_scale.py:52-64): sp (rows, 1025) -> mel (rows, 128). */
int vfx_mel_project(vfx_handle* h, const float* sp, int64_t rows, float* mel, void* stream);

/* torchlibrosa ISTFT via FDomainHelper.istft (fDomainHelper.py:30-32, used unet_v2.py:141):
 * re, im (B, T, 1025) -> wav (B, L). */
int vfx_istft(vfx_handle* h, const float* re, const float* im, int B, int T, int L, float* wav,
              void* stream);

/* stft_hard_lowpass_v0 (tools/dsp/lowpass.py:21-33) of a padded batch of clips in ONE launch: STFT (eps = 1e-8) -> the bins from
 * cut_bins[b] up set to zero -> ISTFT to the clip's length, with no spectrum in memory.  wav (B, L) device, clip b = the first
 * lengths[b] samples of row b; lengths, cut_bins: HOST arrays int[B], n_fft/2 < lengths[b] <= L (reflect padding at the clip's OWN
 * end), cut_bins[b] >= 0 (0: an all-zero clip; 1025 and above: nothing masked).  out (B, L) device, zeros from lengths[b] on; it must
 * not overlap wav.  Row b is bit for bit vfx_istft of (sp * cos, sp * sin), sp / cos / sin = vfx_stft_mel of the clip alone with
 * sp[..., cut_bins[b]:] = 0 and each product rounded to float32; it does not depend on the batch.  Fails, launching nothing, for a
 * NULL pointer, B <= 0, a length outside (n_fft/2, L], a negative cut or overlapping buffers. */
int vfx_stft_lowpass(vfx_handle* h, const float* wav, int B, int L, const int* lengths, const int* cut_bins, float* out, void* stream);

/*
 * The splice of a restored clip onto its band-limited input, for a padded batch of clip pairs at 44.1 kHz, in ONE launch with no spectrum
 * in memory: below the cut-off bin the result is the input, above it the restored clip, with a linear ramp of `ramp` bins between.  Not in
 * the reference (its level half is amp_to_original_f, tools/utils.py:50-55).  x (the input), y (the restored clip): (B, L) device, pair
 * b = the first L_b = lengths[b] samples of row b of both; lengths, cut_bins: HOST arrays int[B], n_fft/2 < lengths[b] <= L, c =
 * cut_bins[b] >= 0; w = ramp >= 0, one value per call; gains: HOST array float[B] of finite values, or NULL: every g = 1.  Per pair, in
 * float32, every product and difference rounded on its own:
 *   gy[n] = g * y[n];  d[n] = x[n] - gy[n];
 *   a[k] = 1 for k <= c - w - 1, 0 for k >= c, float(c - k) / float(w + 1) between (w = 0: the hard mask of vfx_stft_lowpass);
 *   D = vfx_stft_mel's (sp * cos, sp * sin) of d alone (eps = 1e-8), the bins with a = 0 set to +0, each product of a bin with
 *       0 < a < 1 multiplied by a[k], the bins with a = 1 untouched;  r = vfx_istft of D to L_b samples;
 *   out[n] = gy[n] + r[n] for n < L_b, zeros from L_b to L.
 * By linearity this is ISTFT(a STFT(x) + (1 - a) STFT(g y)) with one forward transform per frame, and the band above the seam is g y
 * itself.  Exactly: y == x with g = 1 gives x; y == 0 with w = 0 gives vfx_stft_lowpass(x); c = 0 gives g y.  out (B, L) device must
 * overlap neither x nor y.  Row b is bit for bit the chain of launches above run on the pair alone; it does not depend on the batch, and
 * nothing at or past L_b of either row is read.  More than 128 pairs run as consecutive sub-batches.
 * Fails, naming the clip and launching nothing, for a NULL pointer (gains excepted), B <= 0, a length outside (n_fft/2, L], a negative
 * cut or ramp, a gain that is not finite, or overlapping buffers.
 */
int vfx_stft_splice(vfx_handle* h, const float* x, const float* y, int B, int L, const int* lengths /* HOST */,
                    const int* cut_bins /* HOST */, int ramp, const float* gains /* HOST, or NULL: 1 */, float* out, void* stream);

/*
 * The power of two clips in a band of STFT bins, per pair of a padded batch at 44.1 kHz -- what the level match of the splice compares.
 * a, b: (B, Lmax) device, pair p = the first L_p = lengths[p] samples of row p of both; lengths: HOST array int[B] with n_fft/2 <
 * lengths[p] <= Lmax, or NULL: every clip has Lmax samples; lo_bins, hi_bins: HOST arrays int[B], 0 <= lo <= hi <= 1025.
 *   out[p][0] = sum_t sum_{k = lo}^{hi - 1} (double)|A[k, t]|^2,  out[p][1] = the same of b,  t < L_p / hop + 1,
 * |.| = vfx_stft_mel's float32 magnitude of the clip alone (eps = 1e-8), squared and summed in float64: a lane sums its bins in ascending
 * order, a wave by a fixed tree, the frames by index -- no float atomics, no spectrum in memory.  hi == lo gives zeros.  out: (B, 2)
 * device doubles.  A pair's two numbers do not depend on the batch it is in, on Lmax, or on what lies at or past its end (never read).
 * More than 128 pairs run as consecutive sub-batches.  The frame sums live in the handle's grow-only varlen scratch (see
 * vfx_band_energy).
 * Fails, naming the clip and launching nothing, for a NULL pointer (lengths excepted), B <= 0, a length outside (n_fft/2, Lmax],
 * lo < 0, hi > 1025, hi < lo, or out overlapping a or b.
 */
int vfx_band_power(vfx_handle* h, const float* a, const float* b, int B, int Lmax, const int* lengths /* HOST, or NULL */,
                   const int* lo_bins /* HOST */, const int* hi_bins /* HOST */, double* out /* (B, 2) device */, void* stream);

/*
 * The bandwidth detector of load_wav_energy (tools/utils.py:33-44) for a padded batch of clips at 44.1 kHz: wav (B, Lmax) device
 * floats, clip b = the first L_b = lengths[b] samples of row b; lengths is a HOST array int[B] with n_fft/2 < lengths[b] <= Lmax, or
 * NULL: every clip has Lmax samples.  1 <= hop <= 2048 (librosa.stft's default is 512), 0 < threshold <= 1.  Per clip:
 *   S = the STFT of the clip alone: n_fft 2048, `hop`, periodic Hann, centred frames with reflect padding at the clip's OWN ends,
 *       T_b = L_b / hop + 1 frames, |S| = sqrt(re^2 + im^2) in float32 with NO eps clamp (vfx_stft_phase(eps = 0)'s arithmetic);
 *   e[k] = sum_t log10((double)|S[k, t]| + 1), k = 0 .. 1024, in float64                                       -> energy[b][k]
 *   P[k] = sum_{j<k} e[j], the EXCLUSIVE prefix in ascending k (the loop of utils.py:38-39); total = P[1024]: bin 1024 never counts;
 *   cut_bin[b] = the first k that does not have P[k] < total * threshold (utils.py:41-43).  An all-zero clip gives 0.
 * The cut-off in Hz is int((sample_rate / 2) * (cut_bin / 1025.0)) -- left to the caller.  energy: (B, VFX_BAND_BINS) device doubles,
 * or NULL; cut_bin: B device ints.  A wave sums a fixed number of consecutive frames of one clip, a clip's partial sums are added by
 * index: a clip's 1025 numbers and its bin do not depend on the batch it is in, on Lmax, or on what lies at or past its end (which is
 * never read).  No spectrum is written to memory.  More than 128 clips run as consecutive sub-batches.  The partial sums live in the
 * handle's grow-only varlen scratch: while a hipGraph captured from a plan is alive, a call that would have to grow it fails with a
 * message that says so.
 * Fails, naming the clip and launching nothing, for a NULL wav or cut_bin, B <= 0, or a length, hop or threshold out of range (and
 * for a clip of more than 2^24 frames).
 */
#define VFX_BAND_BINS 1025
int vfx_band_energy(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths /* HOST, or NULL: all Lmax */,
                    int hop, double threshold, double* energy /* (B, 1025) device, may be NULL */,
                    int* cut_bin /* (B) device */, void* stream);

/* Generator.forward of models/gsr_voicefixer.py:86-91 with the mel ResUNet
 * (models/components/unet.py:60-103): linear mel (B, T, 128) >= 0 -> log10 mel (B, T, 128). */
int vfx_resunet_mel(vfx_handle* h, const float* mel_linear, int B, int T, float* logmel_out,
                    void* stream);

/* Generator.forward of models/gsr_voicefixer.py:86-91 with ANY analysis module (`model` = VFX_MODEL_UNET_MEL, _GRU_MEL or
 * _DNN_MEL): linear mel (B, T, 128) >= 0 -> log10 mel estimate (B, T, 128).  frames (HOST array of B, or NULL = all T): clip b
 * has frames[b] <= T live rows, gets what its own call with T = frames[b] computes (the backward GRU starts at ITS last frame)
 * and zero rows past them.  The ResUNet takes frames = NULL only.  The tensor names of the bi_gru / dnn weights are the reference
 * keys without the "generator.analysis_module." prefix ("1.weight", "2.gru.weight_hh_l0_reverse", ...). */
int vfx_analysis_mel(vfx_handle* h, int model, const float* mel_linear, int B, int T, const int* frames, float* logmel_out,
                     void* stream);

/* The analysis module vfx_restore_gsr and vfx_restore_gsr_varlen run: VFX_MODEL_UNET_MEL (the default), _GRU_MEL or _DNN_MEL;
 * its weights must be finalized.  A GRU / DNN module runs once over a whole varlen batch with the clips' frame counts. */
int vfx_select_analysis(vfx_handle* h, int model);

/* UNetResComplex_100Mb.forward of models/components/unet_v2.py:86-148 (ssr_unet / gsr_unet):
 * sp (B, T, 1025), wav (B, L) -> wav_out (B, L). */
int vfx_resunet_spec(vfx_handle* h, const float* sp, const float* wav, int B, int T, int L,
                     float* wav_out, void* stream);

/* voicefixer.Vocoder.__call__ (call site eval_gsr_voicefixer.py:66):
 * linear mel (B, T, 128) -> wav (B, vfx_vocoder_out_len(T)). */
int64_t vfx_vocoder_out_len(vfx_handle* h, int T);
int vfx_vocoder(vfx_handle* h, const float* mel_linear, int B, int T, float* wav_out, void* stream);

/*
 * Whole per-segment body of handler() (eval_gsr_voicefixer.py:47-74) for a batch of
 * equal-length clips: pre -> model -> from_log -> [amp_to_original_f] -> vocoder ->
 * per-clip peak normalise -> trim_center.  wav (B, L) -> wav_out (B, L).
 * flags: bit0 = unify_energy (meta["unify_energy"], tools/utils.py:50-55).
 * logmel_out (B, T, 128) optional (may be NULL): the model's log-mel estimate.
 */
int vfx_restore_gsr(vfx_handle* h, const float* wav, int B, int L, float* wav_out,
                    float* logmel_out, int flags, void* stream);

/*
 * vfx_restore_gsr for a batch of clips of UNEQUAL length (the reference restores one file per call, of any length:
 * evaluation_proc/eval.py:119-134, eval_gsr_voicefixer.py:47-74).  wav, wav_out (B, Lmax); lengths[b] (HOST array) = samples of
 * clip b, n_fft/2 < lengths[b] <= Lmax; logmel_out (B, Lmax / hop + 1, 128) optional.  Every clip gets what its own
 * vfx_restore_gsr(B = 1, L = lengths[b]) call computes -- frames and reflect padding at its own end (fDomainHelper.py:26-28),
 * the ResUNet's zero time padding behind its own last frame (unet.py:75-77), the vocoder stopped at its own length, its own
 * peak normalisation and trim_center -- and zeros past its end in both outputs.  The clips of one call may have ANY lengths
 * (round 6): the mel ResUNet runs once per padded frame count 64 * ceil((lengths[b] / hop + 1) / 64) among them (its clips gathered
 * into a compact batch), the vocoder ONCE over the whole batch.  Hand the batch over with Lmax = (the largest padded frame count)
 * x hop - 1 when many batches follow each other: the launch plans are cached per (B, Lmax).
 */
int vfx_restore_gsr_varlen(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, float* wav_out,
                           float* logmel_out, int flags, void* stream);

/* The spectrogram-domain twin (the per-segment body of handler_ssr_unet, eval_ssr_unet.py:77-114: sp = |STFT(wav)|, model(sp, wav),
 * models/components/unet_v2.py:86-148) for a batch of clips of unequal length: wav, wav_out (B, Lmax), lengths[b] (HOST) samples of
 * clip b.  Per clip the frames and reflect padding of its own length, the trunk's zero padding behind its own last frame, the
 * ISTFT to its own length; zeros past its end.  Same requirement: one padded frame count per call. */
int vfx_restore_ssr_varlen(vfx_handle* h, const float* wav, int B, int Lmax, const int* lengths, float* wav_out, void* stream);

/*
 * vfx_restore_gsr_varlen with the targets of the clips: the restore and the four mel scores handler() returns for a file with a
 * target (eval_gsr_voicefixer.py:56-64), in one call.  wav, lengths, wav_out, logmel_out, flags: as vfx_restore_gsr_varlen, whose
 * launches run unchanged -- both outputs are bit for bit those of that call.  target (B, Lmax) device: clip b of it = its first
 * target_lengths[b] samples (HOST int[B]; NULL: lengths).  metrics_out (B, VFX_N_HANDLER_METRICS) device doubles, per clip over its
 * own T_b = lengths[b] / hop + 1 frames, with
 *   lg  = the model's log10 estimate (logmel_out), unclipped          lin = 10 ** min(lg, 5)   (from_log, in float32)
 *   den = what the vocoder receives: lin, times the amp_to_original_f ratio when flags bit0 is set (float32)
 *   tgt = the target's linear mel: mel(|STFT| clamped at 1e-8) of the target at its own length (float32)
 *   0 mel-lsd             LSD(den, tgt) = mean_t sqrt(mean_f log10(tgt^2 / (den + 1e-12)^2 + 1e-12)^2)
 *   1 mel-sispec          SiSpec(lg, log10(max(tgt, 1e-8)))
 *   2 mel-non-log-sispec  SiSpec(lin, tgt) -- before unify_energy, as the reference takes it
 *   3 mel-ssim            skimage structural_similarity(den, tgt, win_size=7), data_range 2
 * SiSpec(e, g) = 10 log10(pt / (pn + 1e-12) + 1e-12), s = <e,g> / (<g,g> + 1e-8), pt = s^2 <g,g>, pn = max(<e,e> - 2 s <e,g> + pt, 0).
 * Every sum runs in float64 over the clip's own frames in an order fixed by the clip alone: a clip's four numbers do not depend on
 * the batch it is in, and no row at or past its frames is read.  The target mel and the partial sums live in handle scratch that
 * grows only for a call with a target.  Sub-batched as vfx_restore_gsr_varlen.
 * Fails -- naming the clip, before anything is launched -- when target_lengths[b] / hop != lengths[b] / hop (the reference's
 * frame-count mismatch), when a clip has fewer than 7 frames (lengths[b] < 6 hop = 2646: skimage refuses the image), when
 * lengths[b] or target_lengths[b] is outside (n_fft/2, Lmax], and for a NULL target or metrics_out.
 */
#define VFX_N_HANDLER_METRICS 4
int vfx_restore_gsr_varlen_scored(vfx_handle* h, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                                  const int* target_lengths, float* wav_out, float* logmel_out, double* metrics_out, int flags,
                                  void* stream);

/* The spectrogram-domain twin (eval_ssr_unet.py:116-126): vfx_restore_ssr_varlen, whose launches run unchanged, then the same four
 * scores of (est, tgt), est = mel(|STFT| clamped at 1e-8) of the restored clip wav_out[b] at its own length, tgt as above:
 * LSD(est, tgt), SiSpec(log10(max(est, 1e-8)), log10(max(tgt, 1e-8))), SiSpec(est, tgt), SSIM(est, tgt).  Same arithmetic, same
 * failure cases, and still one padded frame count per call. */
int vfx_restore_ssr_varlen_scored(vfx_handle* h, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                                  const int* target_lengths, float* wav_out, double* metrics_out, void* stream);

/*
 * Long-audio chunkers: the two `LambdaOverlapAdd` classes (tools/dsp/overlapadd.py:337-480 and
 * tools/dsp/overlapadd_boxcar.py:338-513) segment a signal, run the network per chunk and stitch.  The
 * network call stays with the caller (all equal-length chunks as ONE batch); these are the two data
 * movements around it.
 *
 * vfx_chunk_gather = F.unfold with zero padding (overlapadd.py:421-428, overlapadd_boxcar.py:436-452):
 *   x (B, L) -> chunks (B, n_chunks, win), chunks[b][k][i] = x[b][k*hop - lead + i], 0 outside [0, L).
 * vfx_chunk_ola = synthesis window (or `scale` when window is NULL) + F.fold (overlapadd.py:455-471):
 *   frames (B, n_chunks, win) -> y (B, L), y[b][n] = sum_k frames[b][k][n + lead - k*hop] * window[..].
 */
int vfx_chunk_gather(vfx_handle* h, const float* x, int B, int L, int win, int hop, int lead,
                     int n_chunks, float* chunks, void* stream);
int vfx_chunk_ola(vfx_handle* h, const float* frames, const float* window, float scale, int B,
                  int n_chunks, int win, int hop, int lead, int L, float* y, void* stream);

/*
 * Streaming sessions: the same two chunkers for signals that arrive in blocks.  A session holds `slots` independent mono
 * streams with all audio on the device: an input ring (capacity samples) and an output ring (out_capacity samples) per slot
 * and, in overlap-add mode, the partial sums of the span that later chunks still change.  Fed in any blocking, a slot's
 * output is bit for bit what the offline pair above gives for its whole signal; which chunk is due, and every ring
 * position, is worked out on the host from sample counts (no call copies anything back from the device to decide).
 *
 *   mode 0, overlap-add: win even, 1 <= hop_or_margin = hop <= win.  Chunk k >= 1 is x[k hop - win, k hop) and is due once
 *     k hop samples are fed; sample n is released when chunk (n + win) / hop is stitched.  capacity >= win.
 *   mode 1, boxcar: hop_or_margin = in_margin >= 0.  Frame 0 is x[0, win + margin), frame k x[k win - margin,
 *     (k + 1) win + margin), due once its last sample is fed; its win output samples are released when it is stitched.
 *     capacity >= win + 2 margin.
 *   window: `win` floats on the DEVICE (copied), or NULL for the factor `scale`.  out_capacity >= win.
 *
 * One step:  push blocks -> next: the due chunks of all slots, ordered by slot, then ascending k, as ONE batch
 * (rows, row_len) with zeros outside the signal -> the caller's network on that batch -> put: the results are stitched and
 * whatever no later chunk can change goes to the output rings -> pop.  A group holds rows of one length only and at most
 * max_rows; what does not fit comes with the following `next` (rows = 0: nothing is due).  A chunk is not handed out
 * while its slot's output ring has no room for what it would release.  vfx_stream_close marks a slot: its remaining
 * chunks, zero-filled past the end -- in boxcar mode the last frame at its own length without a back margin, as the
 * offline class runs it -- then come through the same next / put, after which the slot can be opened again as soon as
 * its output is popped.  A call that is refused (a push that would overrun an input ring, a slot that is not open, a
 * put without a next, ...) changes nothing.
 */
typedef struct vfx_stream vfx_stream;
int vfx_stream_create(vfx_handle* h, int slots, int mode, int win, int hop_or_margin, const float* window, float scale,
                      int64_t capacity, int64_t out_capacity, vfx_stream** st);
int vfx_stream_destroy(vfx_stream* st);
int vfx_stream_open(vfx_stream* st, int* slot);
/* counts[i] samples for slots[i], one after the other in packed_blocks (DEVICE); a slot at most once per call */
int vfx_stream_push(vfx_stream* st, int n, const int* slots, const int64_t* counts, const float* packed_blocks, void* stream);
int vfx_stream_close(vfx_stream* st, int slot);
/* chunks_out (DEVICE): room for max_rows rows of the longest row (win, resp. win + 2 margin); rows * row_len floats are written */
int vfx_stream_next(vfx_stream* st, int max_rows, float* chunks_out, int* rows, int* row_len, void* stream);
/* frames (DEVICE): (rows, row_len) of the outstanding `next`, the network's output for its rows in their order */
int vfx_stream_put(vfx_stream* st, const float* frames, void* stream);
int vfx_stream_available(vfx_stream* st, int slot, int64_t* n);
/* what a push to the slot may hold now: the free part of its input ring, 0 for a slot that is not open */
int vfx_stream_room(vfx_stream* st, int slot, int64_t* n);
/* samples fed to and released by the slot's current (or last) stream */
int vfx_stream_state(vfx_stream* st, int slot, int64_t* fed, int64_t* released);
/* up to max_counts[i] released samples of slots[i], one after the other in packed_out (DEVICE); counts_out[i] were there */
int vfx_stream_pop(vfx_stream* st, int n, const int* slots, const int64_t* max_counts, float* packed_out, int64_t* counts_out,
                   void* stream);

/*
 * Polyphase resampling to the library's rate: librosa.load(path, sr=44100) (tools/utils.py:46-48), i.e.
 * scipy.signal.resample_poly(x, up, down) on float32 input, bit for bit.  up / down are reduced by their gcd first; with
 * M = max(up, down), hl = 10 M, the filter has ntaps = 2 hl + 1 taps, `taps` (DEVICE, fp32) = the taps resample_poly builds:
 * float32(firwin(2 hl + 1, 1 / M, window=('kaiser', 5.0))) * float32(up).  Output n of a clip of n_in samples is
 *   y[n] = sum over ascending k, 0 <= k < n_in, 0 <= n down + hl - k up <= 2 hl, of x[k] * taps[n down + hl - k up]
 * with one fp32 rounding per product and per sum (no FMA), for n < vfx_resample_out_len(n_in) = ceil(n_in up / down).
 *
 * vfx_resample_out_len: -1 for rates <= 0 or a pair whose filter does not fit the kernel (larger than the pairs of 8 .. 96 kHz
 *   <-> 44.1 kHz need; the caller resamples such a pair elsewhere); n_in for the same rate.
 * vfx_resample_window: the input indices [*k0, *k1) that outputs [o0, o0 + n) of a clip of n_in samples read (k0 = k1 = 0 when
 *   none: outputs past the clip's end are zeros); every index in it is read by one of those outputs.
 * vfx_resample: x (B, ldx) holds global input indices [x0, x0 + Lx) of each clip; lens_in (HOST, B) = each clip's whole length
 *   (indices outside [0, lens_in[b]) count as zero); writes global outputs [o0, o0 + n_out) of every clip to y (B, ldy), zeros at
 *   or past a clip's own output length.  Fails when the window lacks an index vfx_resample_window asks for, or for the same rate.
 */
int64_t vfx_resample_out_len(int64_t n_in, int up, int down);
int vfx_resample_window(int64_t n_in, int up, int down, int64_t o0, int64_t n, int64_t* k0, int64_t* k1);
int vfx_resample(vfx_handle* h, const float* x, int B, int64_t ldx, int64_t x0, int64_t Lx, const int64_t* lens_in, int up, int down,
                 const float* taps, int ntaps, float* y, int64_t ldy, int64_t o0, int64_t n_out, void* stream);

/*
 * vfx_resample with a rate pair per clip, for float32 and float64 clips and any pair with max(up, down) <= 65536 after the gcd (what
 * the "stft" low-pass of the degradation simulator, tools/dsp/lowpass.py:135-146, needs at 44.1 / 48 kHz: a drawn cut-off c resamples
 * to int(c / 22050 * 44100) Hz and back).  Row b is scipy.signal.resample_poly(clip b, up, down) of design pair_index[b], bit for bit:
 * the recurrence above in the clip's dtype T, one rounding per product and per sum, with h = fl_T(g T(up)) -- scipy's `h *= up` -- where
 * g = firwin(20 M + 1, 1 / M, window=('kaiser', 5.0)).astype(T), M = max(up, down) after the gcd.  Finite input is the contract.
 *   x (B, ldx) device, float32 (x_f64 = 0) or float64 (1); clip b = the first lens_in[b] samples of row b (HOST int64[B], >= 0);
 *   pair_index HOST int[B], 0 <= pair_index[b] < F;  up, down HOST int[F], as given (reduced inside);  1 <= B, F <= 128;
 *   taps DEVICE, x's dtype: the UNSCALED g of every design back to back; taps_at HOST int64[F]: the element design f starts at (the
 *   down and the up step of one cut-off share M, so they may share one g; not read for a design with up == down after the gcd);
 *   y (B, ldy) device, x's dtype: row b receives outputs [0, n_out), zeros at or past vfx_resample_each_out_len(lens_in[b]); a clip
 *   of a design with up == down is copied.
 * The taps are read from global memory: a call scales each design into a buffer of the handle, phase-major (row phi holds
 * h[phi + j up], so a lane reads one contiguous run), then one launch takes all clips.  The clip and design tables are uploaded on
 * `stream` into a buffer of the handle, grown on demand, so a call is no subject for hipGraph capture.  Fails, launching nothing and
 * leaving y as it is, for a NULL pointer, B or F out of range, an index outside [0, F), a negative length or one past ldx, n_out
 * past ldy, rates <= 0, or a pair past the cap (the message names the clip and its reduced pair).
 * vfx_resample_each_out_len: ceil(n_in up / down) after the gcd; -1 for up or down <= 0, max(up, down) > 65536 after the gcd, or
 *   n_in outside [0, 2^46].
 * vfx_resample, vfx_resample_out_len and vfx_resample_window keep their own, narrower set of pairs.
 */
int64_t vfx_resample_each_out_len(int64_t n_in, int up, int down);
int vfx_resample_each(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lens_in, const int* pair_index,
                      const int* up, const int* down, const void* taps, const int64_t* taps_at, int F, void* y, int64_t ldy, int64_t n_out,
                      void* stream);

/*
 * Zero-phase IIR filtering of a padded batch of clips: scipy.signal.sosfiltfilt(sos, x) per clip (the degradation simulator's
 * low-pass and band-pass, tools/dsp/lowpass.py:58-133), bit for bit, for float32 and float64 input.
 *   x (B, ldx) device, float32 (x_f64 = 0) or float64 (x_f64 = 1); clip b = the first lengths[b] samples of row b (HOST int64[B]);
 *   sos (S, 6) HOST doubles, rows b0 b1 b2 1 a1 a2, 1 <= S <= 16;  zi (S, 2) HOST doubles = scipy.signal.sosfilt_zi(sos);
 *   padlen = 3 * (2 S + 1 - min(#{b2 == 0}, #{a2 == 0})), sosfiltfilt's default; every clip must be longer than padlen;
 *   y (B, ldy) device float64: row b receives the lengths[b] filtered samples, and zeros from there up to ldy.
 * Each clip is extended oddly by padlen samples at both ends in ITS dtype, widened to float64, filtered forward from the state
 * zi * ext[0] and backward from zi * (last forward sample) with x_c = b0 x_n + z0, z0 = (b1 x_n - a1 x_c) + z1, z1 = b2 x_n - a2 x_c
 * per section -- every product and sum rounded on its own -- and trimmed.  Fails, launching nothing, for S or padlen out of range or a
 * clip that is not longer than padlen.  The forward pass lives in a scratch buffer of the handle, grown on demand.
 */
int vfx_sosfiltfilt(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const double* sos, int S,
                    const double* zi, int padlen, double* y, int64_t ldy, void* stream);

/*
 * vfx_sosfiltfilt with a design per clip (the training collator's low-pass, dataloaders/data_module.py:28-70, draws a cut-off, an
 * order and a type for every item): row b is scipy.signal.sosfiltfilt(sos[filter_index[b]], clip b), bit for bit.
 *   x, lengths, y as in vfx_sosfiltfilt;  filter_index HOST int[B], 0 <= filter_index[b] < F;
 *   sos (F, Smax, 6) and zi (F, Smax, 2) HOST doubles, 1 <= F <= 128, 1 <= Smax <= 16: design f is the first sections[f] rows of its
 *   slice (HOST int[F], 1 <= sections[f] <= Smax; the rows past them are not read), zi[f] = scipy.signal.sosfilt_zi of those rows;
 *   padlens HOST int[F]: sosfiltfilt's default padlen of each design; a clip must be longer than the padlen of ITS design.
 * The clips of a call may mix section counts freely: one launch pair (forward, backward) takes up to 128 clips, the blocks of
 * different section counts running side by side.  The bank is uploaded on `stream` into a buffer of the handle, grown on demand,
 * so a call is no subject for hipGraph capture.  Fails, launching nothing and leaving y as it is, for F, Smax, a section count or
 * a padlen out of range, sos[f][s][3] != 1, an index outside [0, F), or a clip that is not longer than its design's padlen (the
 * message names the clip, its length and that padlen).
 */
int vfx_sosfiltfilt_bank(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* filter_index,
                         const double* sos, const double* zi, const int* sections, const int* padlens, int F, int Smax, double* y,
                         int64_t ldy, void* stream);

/*
 * Reverberation of a padded batch of clips: MagicalEffects.reverb_rir (dataloaders/augmentation/magical_effects.py:158-167) per clip,
 * the degradation of the `vctk_reverb` test set -- the full convolution of the clip with a room impulse response, the whole result
 * scaled to a peak of 0.98 when its peak exceeds 0.99, cut back to the clip's length.
 *   x (B, ldx) device float32, clip b = the first lengths[b] samples of row b (HOST int64[B], each >= 1);
 *   rirs (R, ldr) device float32, RIR r = the first rir_lengths[r] taps of row r (HOST int64[R], 1 <= taps <= 2^20);
 *   rir_index HOST int[B]: clip b is convolved with RIR rir_index[b] (NULL: b % R).  A RIR longer than its clip and a one-tap RIR are fine;
 *   y (B, ldy) device float32, ldy >= max(lengths): row b receives lengths[b] samples, and zeros from there up to ldy;
 *   peaks (B) device float32: max |sample| over all lengths[b] + taps - 1 samples of the convolution, tail included, before the
 *   scaling (NaN when a sample is); may be NULL only when normalize is 0.
 * The convolution is in direct form: per output, taps are summed in blocks of 1024 by a float32 fma chain from zero, the block sums
 * are added in float64 in ascending order and rounded to float32 once, so |y - exact| <= (min(taps, 1024) + 2) 2^-24 sum |x||h| + 2^-149
 * per sample, and a clip's result does not depend on the batch it is in.  normalize != 0: a row with (double)peak > 0.99 becomes
 * (y / peak) * 0.98f, a correctly rounded float32 division and a float32 multiplication -- NumPy's arithmetic on a float32 array; a
 * NaN peak leaves the row as it is.  Fails, launching nothing, for an empty clip or RIR, a RIR above 2^20 taps, an index outside
 * [0, R), or ldy < max(lengths).
 */
int vfx_reverb_rir(vfx_handle* h, const float* x, int B, int64_t ldx, const int64_t* lengths, const float* rirs, int R, int64_t ldr,
                   const int64_t* rir_lengths, const int* rir_index, int normalize, float* y, int64_t ldy, float* peaks, void* stream);

/*
 * Noise mixed into a padded batch of clips at a given SNR weight and scale: add_noise_and_scale (form 0), add_noise_and_scale_with_HQ
 * (form 1) and add_noise_and_scale_with_HQ_with_Aug (form 2) of dataloaders/augmentation/base.py:33-118 per clip, the degradation of
 * the noisy test sets and the per-item loop of the training pre-processing.
 *   front, noise, hq, aug (B, ld) device float32, clip b = the first lengths[b] samples of row b of each (HOST int64[B], each >= 1;
 *   what a row holds past them is never read); hq is NULL in form 0, aug is NULL in forms 0 and 1, and they are required otherwise;
 *   noise_weight HOST double[B] = 10 ** (snr / 20) per clip, or NULL: the SNR step is skipped (the reference's snr_l is None);
 *   scale HOST double[B]: the common scale of the clip;
 *   front_out, noise_out, hq_out, aug_out, noisy (B, ld) device float32, each may be NULL when not wanted: row b receives lengths[b]
 *   samples and zeros from there up to ld.  noisy = noise_out + speech_out, the speech being front (forms 0, 1) or aug (form 2).
 * Per clip, in the reference's order: (1) p_x = max |x| of every input; (2) noise / p_noise, and front / p_front (form 0) or hq, front,
 * aug times float(1.0 / max of their peaks) (forms 1, 2); (3) forms 1, 2: level = mean |speech|, and if level > 0.02 the noise is divided
 * by float(mean |noise| / level); (4) noise / float(noise_weight[b]); (5) every returned signal times float(1.0 / peak), peak = max |.|
 * over noise + speech and the returned signals; (6) times float(scale[b]); (7) noisy.
 * Arithmetic: every elementwise step is ONE IEEE float32 operation per sample (a correctly rounded division, division, addition,
 * multiplication, multiplication; never an FMA), and every per-clip scalar is computed in double and rounded to float32 once -- NumPy's
 * arithmetic on a float32 array with a Python-float operand -- so form 0 equals the host function bit for bit.  The two means of step 3
 * are float64 sums over chunks of 4096 samples combined in index order (NumPy sums them pairwise in float32: forms 1 and 2 agree to
 * rounding, not bit for bit).  "max" over several peaks is Python's max() in the reference's argument order, and a NaN sample makes
 * its signal's peak NaN, as np.max does.  A clip's result depends on the clip alone: not on the batch, the row stride or the alignment.
 * Fails, launching nothing, for a form outside 0..2, a pointer the form requires and lacks (or takes and is given), an empty clip, a
 * length above ld, or B above 1024.  Per-clip partial results live in a scratch buffer of the handle, grown on demand.
 */
int vfx_mix_noise(vfx_handle* h, int form, int B, int64_t ld, const int64_t* lengths, const float* front, const float* noise,
                  const float* hq, const float* aug, const double* noise_weight, const double* scale, float* front_out, float* noise_out,
                  float* hq_out, float* aug_out, float* noisy, void* stream);

/*
 * A padded batch of clips quantised to 2 ** bins levels of their own peak: MagicalEffects.quantification
 * (dataloaders/augmentation/magical_effects.py:178-187) per clip, one of the array effects of the training degradation chain.
 *   x (B, ldx) device, float32 (x_f64 = 0) or float64 (x_f64 = 1), clip b = the first lengths[b] samples of row b (HOST int64[B], each
 *   >= 1; what a row holds past them is never read); bins HOST int[B], each in 0..16;
 *   y (B, ldy) device float64: row b receives lengths[b] samples and zeros from there up to ldy;
 *   peaks (B) device in x's dtype, or NULL: max |x| of every clip.
 * Per clip, with level = 2 ** bins and the levels L_j = -1 + (2 j + 1) / level, j < level (exact doubles; the reference's np.linspace
 * gives the same values bit for bit): p = max |x| in x's dtype (NaN if a sample is); s = x / p, one correctly rounded division in x's
 * dtype; k = the number of levels below (double)s, a NaN s counting as above all of them -- np.digitize(s, L, right=True); idx = k - 1,
 * and idx = -1, for a sample at or below the lowest level, is the TOP level as NumPy's negative index makes it (the negative peak -p
 * comes out as +(1 - 1 / level) p); y = L_idx * (double)p, one double multiplication.  k is settled by comparisons of s with the exact
 * levels, so y equals the host function bit for bit; zero, infinite and NaN peaks take the same steps (a silent clip gives zeros, a
 * clip with a NaN gives NaN throughout).  A clip's result depends on the clip alone: not on the batch, the row stride or the alignment.
 * Fails, launching nothing and leaving y as it is, for B outside 1..1024, an empty clip, a length above ldx or ldy, bins outside
 * 0..16, or a NULL other than peaks.
 */
int vfx_quantize(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int* bins, double* y,
                 int64_t ldy, void* peaks, void* stream);

/*
 * A stretch of every clip of a padded batch silenced and its two edges smoothed: MagicalEffects.time_dropout
 * (magical_effects.py:169-176) with tools/others/audio_op.py:152-174 `smooth` per clip.
 *   x, lengths as in vfx_quantize; starts, ends HOST int64[B]: the sample range [start, end) of clip b, 0 <= start <= end (the
 *   reference's int(length * start) and int(length * start + length * trunk_length)); an end past the clip is cut to its length;
 *   smooth HOST double[96 * 25]: the matrix M of `smooth` with its defaults -- the 96 samples it writes are M times the 25 knots it
 *   reads, every fourth sample of the 100 around the centre (cubic interpolation is linear in the knots); kept in a device buffer of the
 *   handle and uploaded again only when its contents change;
 *   y (B, ldy) device in x's dtype, not overlapping x: row b receives lengths[b] samples and zeros from there up to ldy.
 * Per clip of n samples: y = x with y[start : min(end, n)] = 0; then for c = start and c = end, in that order, if c >= 50 and
 * n - c >= 50: the knots y[c - 50 + 4 i], i < 25, are read after everything before them has been written (the second patch may overlap
 * the first and the zeroed range), and y[c - 50 + t] = sum_i M[t][i] knot_i for t < 96, the sum in double in ascending i, rounded once
 * to x's dtype.  Outside the two patches y is x or zero, bit for bit.  A clip's result depends on the clip alone.
 * Fails, launching nothing and leaving y as it is, for B outside 1..1024, an empty clip, a length above ldx or ldy, start < 0,
 * end < start, or a NULL argument.
 */
int vfx_time_dropout(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths, const int64_t* starts,
                     const int64_t* ends, const double* smooth, void* y, int64_t ldy, void* stream);

/*
 * The fully specified part of MagicalEffects' sox chain (dataloaders/augmentation/magical_effects.py:41-64, 131-152) on a padded batch
 * of float32 clips, a program per clip: the biquads low_pass, high_pass, bass and treble, clip and reverse.  Restated from published
 * definitions and not pinned against sox; simulate.chain_effects is the host form a clip's result equals bit for bit.
 *   x (B, ldx) device float32, clip b = the first lengths[b] samples of row b (HOST int64[B], each >= 1);
 *   ops (B, K) HOST ints, 1 <= K <= 8: the steps of clip b in order, VFX_CHAIN_END ends a program short of K;
 *   coef (B, K, 5) HOST doubles: b0 b1 b2 a1 a2 (a0 = 1) of a VFX_CHAIN_BIQUAD step, the factor in the first slot of a VFX_CHAIN_CLIP step;
 *   y (B, ldy) device float32, not overlapping x: row b receives lengths[b] samples and zeros from there up to ldy.
 * A run is a maximal stretch of biquads and reverses: entering it the clip is widened to float64 and limited to [-1, 1 - 2^-31]; a
 * biquad is x_c = b0 x_n + z0, z0 = (b1 x_n - a1 x_c) + z1, z1 = b2 x_n - a2 x_c from a zero state -- every product and sum rounded on
 * its own --, its output limited to that range again while the state keeps the unlimited value; a reverse flips the clip; the run's
 * result is rounded once to float32.  A clip step clamps the float32 clip to [min * (float)factor, max * (float)factor], float32
 * products of the minimum and maximum of the clip as it stands.  sox's rounding to multiples of 2^-31 is not modelled.
 * Every clip has its own program; a run of up to four biquads is one launch whatever the programs of the batch, and a clip's result
 * depends on the clip alone: not on the batch, the row stride, the alignment or its neighbours' programs.  A sample that is not
 * finite changes no other clip; what its own clip becomes is not specified (the limit and the clamp send a NaN to their lower
 * bound, where the host form keeps it).  Intermediate clips live in a scratch buffer of the handle, grown on demand, and the programs are uploaded on `stream`, so
 * a call is no subject for hipGraph capture.  Fails, launching nothing and leaving y as it is, for B outside 1..1024, an empty clip,
 * a length above ldx or ldy, K outside 1..8, an unknown op, more than four biquads in one run, or a NULL argument.
 */
enum { VFX_CHAIN_END = 0, VFX_CHAIN_BIQUAD = 1, VFX_CHAIN_CLIP = 2, VFX_CHAIN_REVERSE = 3 };
int vfx_effect_chain(vfx_handle* h, const float* x, int B, int64_t ldx, const int64_t* lengths, const int* ops, const double* coef, int K,
                     float* y, int64_t ldy, void* stream);

/*
 * The peak-threshold silence functions of the reference's data preparation (tools/others/audio_op.py:79-150) for a padded batch of
 * clips: x (B, ldx) device, float32 (x_f64 = 0) or float64 (1), clip b = the first n_b = lengths[b] samples of row b; lengths is a HOST
 * array.  Everything is decided by window peaks max |x[i]| over windows of one clip, compared with `threshold` IN THE CLIP'S DTYPE: the
 * threshold is rounded to float32 first for float32 clips, as NumPy >= 2 compares a Python scalar with a float32 array.  A NaN sample
 * makes its windows' peaks NaN, which is neither < nor > the threshold, as the reference's comparisons come out.
 *
 * vfx_trim_bounds: trim_tail_empty (`which` = VFX_TRIM_TAIL), trim_head_empty (VFX_TRIM_HEAD) or trim_empty (VFX_TRIM_BOTH) as the
 * sample range [start[b], stop[b]) the function keeps of clip b, or start = stop = -1 where it returns None.  seg = int(sample_rate *
 * frame_length).
 *   tail  n < seg -> None.  The windows lie on the grid that ENDS at n (origin n % seg, stride = width = seg); from the last one, while
 *         the window's end L > seg and its peak < threshold, L -= seg.  L < seg -> None; L == n -> [0, n); else [0, L - seg): the
 *         reference drops one further segment, and L == seg leaves the EMPTY clip [0, 0), which is not None.
 *   head  on a clip of m samples: windows [k seg, (k + 1) seg) from 0; s = 0, and while s < m - seg and the peak < threshold, s += seg.
 *         s >= m - seg -> None (every m <= seg among them); s == 0 -> [0, m); else [s - seg, m): one quiet segment stays.
 *   both  tail, then head on the tail's result (m = its stop); None if either is.
 * Lengths 0 <= n_b <= ldx; a clip of length 0 gives None.
 *
 * vfx_long_empty: has_long_empty.  flag[b] = 1 if any window [L - seg, L), L = n, n - step, n - 2 step, ... while L > seg, has a peak
 * < threshold, else 0 (the reference: seg = int(sample_rate * 3), step = sample_rate, threshold 400).  Lengths 0 <= n_b <= ldx.
 *
 * vfx_active_frames: get_all_active_segment_index.  The clip is reflect-padded by `shift` samples on both sides (np.pad(...,
 * mode="reflect"): the edge sample is not repeated); frames of `frame` samples every `shift` start at padded index 0 while a frame fits
 * into n + 2 shift samples: vfx_active_frames_count frames (host arithmetic; -1 for arguments out of range).  labels[b][k] = 1 where
 * frame k's peak > threshold (strictly: is_valid_signal), else 0; the rest of the row, up to ldf, is 0.  counts (may be NULL): the frame
 * count of each clip.  Lengths shift < n_b <= ldx (one reflection), ldf >= every clip's frame count.
 *
 * One wave takes one window (a 20-ms window is 3.5 kB); a second kernel decides a clip from its peaks by index.  A clip's results do
 * not depend on the batch it is in, on ldx, on the rows' alignment or on what lies at or past its end, which is never read.  More than
 * 128 clips run as consecutive sub-batches.  The peaks live in the handle's grow-only varlen scratch: while a hipGraph captured from a
 * plan is alive, a call that would have to grow it fails with a message that says so.
 * Each call fails, naming the clip where there is one and launching nothing, for a NULL pointer (counts excepted), B outside 1..1024,
 * a length out of range, seg, step, frame or shift <= 0, an unknown `which`, or a threshold that is not finite.
 */
enum { VFX_TRIM_TAIL = 0, VFX_TRIM_HEAD = 1, VFX_TRIM_BOTH = 2 };
int vfx_trim_bounds(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths /* HOST */, int64_t seg,
                    double threshold, int which, int64_t* start /* (B) device */, int64_t* stop /* (B) device, -1 / -1 = None */,
                    void* stream);
int vfx_long_empty(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths /* HOST */, int64_t seg,
                   int64_t step, double threshold, int* flag /* (B) device */, void* stream);
int vfx_active_frames(vfx_handle* h, const void* x, int x_f64, int B, int64_t ldx, const int64_t* lengths /* HOST */, int64_t frame,
                      int64_t shift, double threshold, uint8_t* labels /* (B, ldf) device */, int64_t ldf,
                      int64_t* counts /* (B) device, may be NULL */, void* stream);
int64_t vfx_active_frames_count(int64_t n, int64_t frame, int64_t shift);

/*
 * Spectral metrics of the evaluation handlers, per clip, without leaving the device
 * (evaluation_proc/metrics.py:83-95 `lsd`, `sispec`; evaluation_proc/utils.py:81-101 `energy_unify`,
 * `pow_p_norm`; used at eval_gsr_voicefixer.py:56-64):  est, target (B, T, F) -> out (B, 2),
 *   out[b][0] = LSD(est, target)    (linear-scale inputs, "mel-lsd"),
 *   out[b][1] = SiSpec(est, target) in dB (log-scale inputs for "mel-sispec", linear for "mel-non-log-sispec").
 * The reference returns the batch mean of these.
 */
int vfx_spectral_metrics(vfx_handle* h, const float* est, const float* target, int B, int T, int F,
                         float* out, void* stream);

/*
 * The scores of AudioMetrics.evaluation (evaluation_proc/metrics.py:25-106) for a padded batch of (est, target) waveform pairs at
 * 44.1 kHz: est, target (B, Lmax) device, pair b = the first lengths[b] samples of row b; lengths is a HOST array int[B] with
 * 2646 <= lengths[b] <= Lmax (at least 7 STFT frames: skimage rejects a smaller SSIM image).  out (B, 9) device doubles, in this order:
 *   0 sisdr                     speechmetrics sisdr over the whole clip (metrics.py:59): a = (eps + <t,e>) / (<t,t> + eps),
 *                               10 log10((eps + |a t|^2) / (eps + |e - a t|^2)), eps = DBL_EPSILON
 *   1 lsd                       AudioMetrics.lsd (metrics.py:83-87) of the magnitude spectrograms (metrics.py:75)
 *   2 non_log_sispec            AudioMetrics.sispec (metrics.py:89-95) of the magnitudes (metrics.py:76)
 *   3 sispec                    ... of to_log of the magnitudes, log10(max(x, 1e-8)) (metrics.py:77, utils.py:60-61)
 *   4 ssim                      AudioMetrics.ssim (metrics.py:97-106): skimage structural_similarity(win_size=7) of the (T, 1025) image
 *   5-8 final_mel_lsd, final_non_log_mel_sispec, final_mel_sispec, final_mel_ssim: the same four of the (T, 128) mel images
 *                               (metrics.py:80-83; MelScale(n_mels=128, sample_rate=44100, n_stft=1025) of the magnitudes)
 * The magnitude is |STFT| with n_fft 2048, hop 441, periodic Hann, centre reflect padding and no eps clamp (librosa.stft,
 * metrics.py:45): T = 1 + lengths[b] / 441 frames per clip.  Every per-clip sum is in float64, in an order fixed by the clip alone:
 * a clip's nine numbers do not depend on the batch it is in nor on Lmax.  The call sub-batches its clips so that its workspace,
 * owned by the handle and grown only when needed, stays under 256 MiB (more only when ONE clip needs more).
 */
#define VFX_N_AUDIO_METRICS 9
int vfx_audio_metrics(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, double* out,
                      void* stream);
/*
 * The same nine scores for test sets at `rate` Hz, the two rates the reference has a front end for (evaluation_proc/metrics.py:37-51):
 *   44100  exactly vfx_audio_metrics (which forwards here), bit for bit
 *   16000  |STFT| with n_fft 743, hop 160, periodic Hann, centre reflect padding (librosa.stft: an odd n_fft pads 371 samples on each
 *          side, so T = 1 + (lengths[b] - 1) / 160 frames) -> the (T, 372) image, and MelScale(n_mels=80, sample_rate=16000, n_stft=372)
 *          of it -> the (T, 80) image; 961 <= lengths[b] <= Lmax (7 frames).  The transform is a DFT-matrix product on the f32-input
 *          MFMA, one f32 fma chain over the 743 samples of a frame in ascending order (stft_dft.hip); its tables belong to the handle,
 *          are built on the first call and need no particular vfx_config.  The filterbank is the HTK table evaluated in float64 unless
 *          a (372, 80) tensor "mel16k.fb" was loaded into VFX_MODEL_FRONTEND.
 * Any other rate is an error.  Scores, sub-batching, workspace and batch independence are vfx_audio_metrics'.
 */
int vfx_audio_metrics_rate(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int rate,
                           double* out, void* stream);

/*
 * STOI, the short-time objective intelligibility measure (Taal, Hendriks, Heusdens, Jensen, IEEE TASLP 2011; restated from the paper,
 * the authors' MATLAB and pystoi's stoi(extended=False) -- not pinned against the pystoi package), for a padded batch of (est, target)
 * waveform pairs: est, target (B, Lmax) device floats, pair b = the first lengths[b] samples of row b; lengths is a HOST array int[B]
 * with 1 <= lengths[b] <= Lmax.  target is the clean signal, est the processed one: the score is not symmetric.  out: B device doubles.
 *   1  both signals go to 10 kHz by scipy.signal.resample_poly(x, up, down, window=taps): up / down = 10000 / fs (reduced by their gcd
 *      here), taps = ntaps DEVICE doubles, the filter ALREADY multiplied by up, ntaps odd.  up == down: the clips are at 10 kHz, taps is
 *      not read and may be NULL.  The resampler takes a reduced up <= 1024, down <= 32768 and ntaps <= 2^20; anything beyond is refused
 *      with an error that names the limit, never truncated.
 *   2  silent-frame removal: w = hanning(258)[1:-1], frames of 256 at range(0, n - 256, 128) (the authors' 1:hop:(n - N): the last
 *      aligned frame is NOT taken), e = 20 log10(|w . target frame| + EPS), kept when max(e) - 40 - e < 0, the kept windowed frames of
 *      both signals overlap-added at hop 128
 *   3  STFT of both by the same window and frame rule (kept - 1 frames), 512-point; fewer than 30 frames: the score is 1e-5
 *   4  15 third-octave bands from 150 Hz: the square root of the summed |X|^2 of rFFT bins [7,9) [9,11) [11,14) [14,17) [17,22) [22,27)
 *      [27,34) [34,43) [43,55) [55,69) [69,87) [87,109) [109,138) [138,174) [174,219)
 *   5  per segment of 30 frames and band: a = |x| / (|y| + EPS), y' = min(a y, x (1 + 10^(15/20))), both minus their means and divided
 *      by (their norm + EPS), the inner product; out[b] = the mean over segments and bands.  EPS = 2^-52.
 * Float64 from the first multiply on, every sum in an order fixed by the clip alone: a clip's score does not depend on the batch it is
 * in nor on Lmax; nothing at or past a clip's length is read.  The workspace is the one of vfx_audio_metrics (sub-batched under 256 MiB).
 */
int vfx_stoi(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int up, int down,
             const double* taps, int ntaps, double* out, void* stream);

/*
 * BSS Eval v4 "images" SDR, ISR and SAR (Vincent, Gribonval, Fevotte, IEEE TASLP 2006; the SiSEC 2018 form that speechmetrics calls
 * with window = inf), specialised to one source, one channel and one window over the whole file; restated from this definition --
 * not pinned against the museval package -- for a padded batch of (est, target) waveform pairs: est, target (B, Lmax) device floats,
 * pair b = the first n = lengths[b] samples of row b; lengths is a HOST array int[B] with 1 <= lengths[b] <= Lmax.  flen = L, the taps
 * of the allowed distortion filter: a multiple of 16 in [16, 512] (the reference uses 512); anything else is refused before the first
 * launch.  out: (B, 3) device doubles, sdr, isr, sar.  With r the target and e the est, both promoted to float64:
 *   1  a[k] = sum_t r[t] r[t + k], k < L; terms whose index falls outside [0, n) are zero
 *   2  d[k] = sum_t e[t] r[t - k], k < L, likewise (the products of two floats are exact in float64: only the summation rounds)
 *   3  (toeplitz(a) + EPS I) c = d, EPS = 2^-52, by the Levinson recursion
 *   4  P[t] = sum_k c[k] r[t - k], t < n + L - 1; r and e are zero-padded to n + L - 1
 *   5  Err = sum r^2, Eer = sum (e - r)^2, Epr = sum (P - r)^2, Epp = sum P^2, Eep = sum (e - P)^2 over t < n + L - 1
 *   6  sdr = 10 log10(Err / Eer), isr = 10 log10(Err / Epr), sar = 10 log10(Epp / Eep); a denominator that is exactly 0 gives +inf; if
 *      every sample of r, or every sample of e, is exactly 0, all three are NaN (the silent-source rule)
 * Float64 from the first multiply on (the correlations and the projection on the f64 MFMA), every sum in an order fixed by the clip
 * alone -- slabs of VFX_BSSEVAL_SLAB samples cut from the clip's own extent, combined in ascending order: a clip's scores do not depend
 * on the batch it is in, on Lmax, nor on what lies at or past its length in its row; nothing there is read.  The workspace is the one
 * of vfx_audio_metrics (sub-batched under 256 MiB).
 */
#define VFX_BSSEVAL_SLAB 8192
int vfx_bsseval(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths, int flen, double* out,
                void* stream);

/*
 * The validation losses of the training scripts, forward values only (no gradient), for a padded batch of (est, target) waveform pairs
 * at 44.1 kHz: est, target (B, Lmax) device floats, pair b = the first L_b = lengths[b] samples of row b; lengths is a HOST array int[B]
 * with n_fft/2 < lengths[b] <= Lmax, or NULL: every clip has Lmax samples.  out: (B, VFX_N_SPEC_LOSSES) device doubles, per clip over its
 * own L_b samples and T_b = L_b / hop + 1 frames:
 *   0 l1_wav     mean |e - t|                                 (nn.L1Loss of the waveforms)
 *   1 l1_sp      mean over T_b x 1025 of | |STFT e| - |STFT t| |          (tools/pytorch/losses.py:192-204 L1_Sp, eps 1e-8)
 *   2 l1_log_sp  the same mean of | log10 |STFT e| - log10 |STFT t| |     (losses.py L1_Log_Sp)
 * |STFT .| = sqrt(max(re^2 + im^2, 1e-8)) is bit for bit vfx_stft_phase(eps = 1e-8)'s magnitude of the clip alone (frames and
 * reflection of its own length).  A difference of columns 0 and 1 is ONE float32 subtraction, its absolute value widened to double; the
 * logarithms of column 2 are taken in float64.  Every sum is in float64 in an order fixed by the clip alone (per frame, per chunk of
 * 4096 samples, then by index): a clip's three numbers do not depend on the batch it is in nor on Lmax, est == target gives exactly 0,
 * and nothing at or past a clip's length is read.  No spectrogram is written to memory (one fused launch transforms both clips).  More
 * than 128 clips run as consecutive sub-batches.  The partial sums live in the handle's grow-only varlen scratch: while a hipGraph
 * captured from a plan is alive, a call that would have to grow it fails with a message that says so.
 * Fails, naming the clip and launching nothing, for a NULL pointer, B <= 0, or a length out of range.
 */
#define VFX_N_SPEC_LOSSES 3   /* 0 l1_wav  1 l1_sp  2 l1_log_sp */
int vfx_spec_losses(vfx_handle* h, const float* est, const float* target, int B, int Lmax, const int* lengths,
                    double* out /* (B, 3) device */, void* stream);

/*
 * Column 0 of vfx_spec_losses for tensors that are not waveforms (nn.L1Loss of two log-mel images): a, b (B, ld) device floats, row r =
 * its first counts[r] elements (HOST int[B], 1 <= counts[r] <= ld; NULL: all ld) -> out[r] = mean |float32(a_i - b_i)|, B device
 * doubles, by the same chunked float64 sums (a row's number depends on the row alone).  Fails, launching nothing, for a NULL pointer,
 * B <= 0, ld outside (0, 2^31) or a count out of range.
 */
int vfx_l1_rows(vfx_handle* h, const float* a, const float* b, int B, int64_t ld, const int* counts, double* out, void* stream);

/*
 * val_l of VoiceFixer's validation_step (models/gsr_voicefixer.py:264-277) per clip of a padded batch, without the vocoder:
 *   val_l[b] = mean over T_b x 128 of | float32(lg - tlog) |,  lg = the selected analysis module's log10 estimate of clip b -- the
 *   first half of vfx_restore_gsr_varlen: the same launches, plans and scratch --, tlog = to_log(mel(target b)) at the target's own
 *   length (vfx_stft_mel(log10_mel = 1)).
 * wav, target (B, Lmax) device floats; lengths HOST int[B]; target_lengths HOST int[B] or NULL (= lengths); logmel_out (B, T, 128)
 * device or NULL: bit for bit vfx_restore_gsr_varlen's; val_l: B device doubles.  The sum is in float64 over chunks of 4096 values cut
 * from the clip's own first row, then by index: a clip's val_l does not depend on the batch.  Any mix of lengths; more than 128 clips
 * run as consecutive sub-batches.  Only the analysis module's weights have to be finalized.
 * Fails, naming the clip and launching nothing, for a NULL wav, target, lengths or val_l, B <= 0, a length of a clip or of a target
 * outside (n_fft/2, Lmax], or a target whose frame count differs from its clip's.
 */
int vfx_validate_gsr_varlen(vfx_handle* h, const float* wav, const float* target, int B, int Lmax, const int* lengths,
                            const int* target_lengths, float* logmel_out /* optional */, double* val_l /* (B) device */, void* stream);

/* Read-and-clear the sticky device flags (synchronises `stream`). */
int vfx_take_flags(vfx_handle* h, void* stream, int* flags_out);
/* ... only the bits in `mask` (VFX_FLAG_*): the others stay raised for a later check. */
int vfx_take_flags_masked(vfx_handle* h, void* stream, int mask, int* flags_out);

/*
 * Turns for work the library does not enqueue itself.  Calls of this library on different streams of one device take turns on
 * the GPU timeline (see "Conventions"); a call made during a stream capture is exempt, so the REPLAY of a hipGraph captured
 * from such calls must be bracketed by the caller when anything of this library may run on another stream of the device at
 * the same time:  vfx_turn_begin(device, s); hipGraphLaunch(graph, s); vfx_turn_end(device, s);  (Engine.replay does this).
 * begin makes `s` wait for the end of the device's previous turn, end leaves the event the next call waits for.  Not needed
 * when everything of a process runs on one stream per device.
 */
int vfx_turn_begin(int device, void* stream);
int vfx_turn_end(int device, void* stream);

/*
 * Live kernel timing for the roofline report: between vfx_profile_begin and vfx_profile_end
 * every tap-convolution launch is bracketed by HIP events on its own stream.
 * vfx_profile_end synchronises and returns the number of launches, the sum of their
 * durations (ms) and of their algorithmic FLOPs (2*M*Cout*K); out pointers may be NULL.
 */
int vfx_profile_begin(vfx_handle* h);
int vfx_profile_end(vfx_handle* h, int64_t* launches, double* total_ms, double* total_flops);

#ifdef __cplusplus
}
#endif
#endif /* VFX_H_ */
