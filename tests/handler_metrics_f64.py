"""float64 numpy restatement of the four mel scores a handler returns for a file with a target (eval_gsr_voicefixer.py:59-64,
eval_ssr_unet.py:121-126), built from audio_metrics_f64's lsd / sispec / ssim / to_log.  One clip: (T, 128) images.

KEYS is the column order of vfx_restore_gsr_varlen_scored / vfx_restore_ssr_varlen_scored (include/vfx.h)."""
import numpy as np

import audio_metrics_f64 as am

KEYS = ("mel-lsd", "mel-sispec", "mel-non-log-sispec", "mel-ssim")


def from_log(lg):
    """pytorch_util.py:161-163 in float64: 10 ** min(lg, 5)."""
    return 10.0 ** np.minimum(np.asarray(lg, np.float64), 5.0)


def gsr_scores(lg, lin, den, tgt):
    """The GSR handler's operand mix: lg the model's log10 estimate, lin = from_log(lg), den what the vocoder receives (lin, scaled by
    amp_to_original_f when unify_energy is on), tgt the target's linear mel -> the four scores in KEYS order."""
    lg, lin, den, tgt = (np.asarray(a, np.float64) for a in (lg, lin, den, tgt))
    return np.array([am.lsd(den, tgt), am.sispec(lg, am.to_log(tgt)), am.sispec(lin, tgt), am.ssim(den, tgt)])


def ssr_scores(est, tgt):
    """The SSR handler's: all four of the restored clip's mel and the target's."""
    est, tgt = np.asarray(est, np.float64), np.asarray(tgt, np.float64)
    return np.array([am.lsd(est, tgt), am.sispec(am.to_log(est), am.to_log(tgt)), am.sispec(est, tgt), am.ssim(est, tgt)])
