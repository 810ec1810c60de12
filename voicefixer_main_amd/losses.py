"""tools/pytorch/losses.py on the device: the L1 family of `get_loss_function`, FORWARD VALUES ONLY.

The callables here return numbers, not graph nodes: nothing is differentiable and no training step is built on them.  They exist
to re-rank checkpoints and to check a converted checkpoint against the `val_l` in its file name (validation_step of
models/ssr_unet.py and models/gsr_unet.py uses `get_loss_function("l1_sp")`, models/gsr_voicefixer.py `"l1"` on log-mel images).

Every callable is `(output, target, lengths=None) -> 0-dim float64 tensor on the device`:

    l1, l1_wav          mean |output - target|                              (losses.py:273-279; any shape)
    l1_sp               mean | |STFT output| - |STFT target| |, eps 1e-8    (losses.py:192-204)
    l1_log_sp           the same of log10 of both                           (losses.py:178-190)
    l1_wav_l1_sp        alpha_t l1_wav + (1 - alpha_t) l1_sp / sqrt(2048)   (losses.py:206-237, alpha_t = 0.85)
    l1_wav_l1_log_sp    ... with l1_log_sp                                  (losses.py:239-270)

Waveforms are (B, L), (B, 1, L), (B, L, 1) or (L,).  The library computes one value per clip over the clip's own samples and frames
(Engine.spec_losses, Engine.l1_rows: float64 sums in an order fixed by the clip alone); the callable returns their mean, taken in
float64 on the device.  For equal lengths that is the reference's batch mean; with `lengths` (a padded batch, clip b = its first
lengths[b] samples) it is the mean of what the reference gives clip by clip.  Every other name of the reference's table raises
NotImplementedError.
"""
import math

import torch

ALPHA_T = 0.85          # the default of L1_Wav_L1_Sp.__call__ / L1_Wav_L1_Log_Sp.__call__
WINDOW_SIZE = 2048      # their self.window_size: sp_loss /= sqrt(window_size)

# name -> (column of Engine.spec_losses that is the spectrogram term or None, whether the waveform L1 is mixed in)
SUPPORTED = {
    "l1": (None, True),
    "l1_wav": (None, True),
    "l1_sp": (1, False),
    "l1_log_sp": (2, False),
    "l1_wav_l1_sp": (1, True),
    "l1_wav_l1_log_sp": (2, True),
}
# the rest of the reference's table (losses.py:52-80)
UNSUPPORTED = ("sisnr", "sispec", "simelspec", "sispeclog", "snr", "bce", "wm44k", "lsd")


def mix_weights(alpha_t=ALPHA_T, window_size=WINDOW_SIZE):
    """(weight of l1_wav, weight of the spectrogram L1) of the two mixed losses: alpha_t, (1 - alpha_t) / sqrt(window_size)."""
    return float(alpha_t), (1.0 - float(alpha_t)) / math.sqrt(window_size)


def _waveform_rows(x):
    """(B, L), (B, 1, L), (B, L, 1) or (L,) -> (B, L); None for any other shape (not a waveform)."""
    if x.dim() == 1:
        return x[None]
    if x.dim() == 2:
        return x
    if x.dim() == 3 and x.shape[1] == 1:
        return x[:, 0]
    if x.dim() == 3 and x.shape[2] == 1:
        return x[:, :, 0]
    return None


class Loss:
    """One entry of the table: `loss(output, target, lengths=None)`.  `engine`: the Engine to run on; None = one made on the
    device of the first `output`."""

    def __init__(self, loss_type, engine=None):
        self.loss_type = loss_type
        self.sp_column, self.with_wav = SUPPORTED[loss_type]
        self.engine = engine

    def _engine(self, output):
        if self.engine is None:
            from .engine import Engine
            self.engine = Engine(output.device if isinstance(output, torch.Tensor) and output.is_cuda else "cuda:0")
        return self.engine

    def __call__(self, output, target, lengths=None, alpha_t=ALPHA_T):
        eng = self._engine(output)
        if not isinstance(output, torch.Tensor):
            output = torch.as_tensor(output)
        if not isinstance(target, torch.Tensor):
            target = torch.as_tensor(target)
        if tuple(output.shape) != tuple(target.shape):
            raise ValueError("%s: output %s and target %s differ in shape" % (self.loss_type, tuple(output.shape), tuple(target.shape)))
        if self.sp_column is None:       # nn.L1Loss: any shape, row b = everything of batch entry b
            o, t = _waveform_rows(output), _waveform_rows(target)
            if o is None:                # not a waveform: the log-mel case, (B, T, F) or the reference's (B, 1, T, F)
                o, t = output, target
                if o.dim() == 4 and o.shape[1] == 1:
                    o, t = o[:, 0], t[:, 0]
            counts = None
            if lengths is not None:      # lengths count entries of dimension 1 (samples of a waveform, frames of a (B, T, F) image)
                inner = 1
                for n in o.shape[2:]:
                    inner *= int(n)
                counts = [int(v) * inner for v in lengths]
            return eng.l1_rows(o, t, counts).mean()
        o, t = _waveform_rows(output), _waveform_rows(target)
        if o is None:
            raise ValueError("%s: takes waveforms (B, L), (B, 1, L), (B, L, 1) or (L,), got %s" % (self.loss_type, tuple(output.shape)))
        cols = eng.spec_losses(o, t, lengths)            # (B, 3) float64 on the device
        if not self.with_wav:
            return cols[:, self.sp_column].mean()
        w_wav, w_sp = mix_weights(alpha_t)
        return (w_wav * cols[:, 0] + w_sp * cols[:, self.sp_column]).mean()


def get_loss_function(loss_type, engine=None):
    """losses.get_loss_function for the L1 family (module docstring): forward values only, no gradient.  Any other name of the
    reference's table raises NotImplementedError naming it; a name it does not have, ValueError."""
    if loss_type in SUPPORTED:
        return Loss(loss_type, engine)
    if loss_type in UNSUPPORTED:
        raise NotImplementedError("get_loss_function: '%s' is not implemented on the device (implemented: %s)"
                                  % (loss_type, ", ".join(sorted(SUPPORTED))))
    raise ValueError("get_loss_function: unknown loss '%s'" % (loss_type,))
