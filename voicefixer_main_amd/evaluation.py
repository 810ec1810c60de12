"""The reference's `inference()` and `evaluation()` (evaluation_proc/eval.py:89-135, 142-221) on the batched, scored restore.

`inference` restores every file of a test-set list and writes `<save_dir>/<testset>/<basename>` with the handler's scores as
`<basename minus .wav>.json` beside it (`{}` for a line without a target), as the reference does one handler call per file.  Here
a file that is ONE segment goes through `model.restore_scored_list` (a padded batch per call, the four mel scores computed on the
device inside it: Engine.restore_gsr_varlen_scored / restore_ssr_varlen_scored), or `model.restore_list` when its line has no
target.  A file is batched iff

  * input and target are 44.1 kHz wav files the handlers' reader takes (`handlers.load_wav`: PCM of 1, 2 or 4 bytes);
  * both hold more than 1024 samples (reflect padding) and at most 60 s, i.e. one segment of the handler's loop;
  * the target has at least 2646 samples (7 STFT frames: the SSIM window) and the input's frame count (len // 441)

-- for a line without a target the first two, of the input.  Every other file goes through the per-file handler
(`handlers.handler_gsr_voicefixer` / `handler_ssr_unet`) unchanged: its errors (a frame-count mismatch, an unreadable file) and
its multi-segment semantics (the last segment's scores win) stay the handler's.

`evaluation` is `inference`, then `metrics.aggregate_score` per test set, then `metrics.gather_score`.  One process, no progress
bar, no process pool; sharding a scored set over ranks is not implemented (restore_scored_list raises).
"""
import inspect
import logging
import os
import random
import time
import wave

from . import clips, handlers, metrics, models

SAMPLE_RATE = 44100
MIN_SAMPLES = 1024 + 1                              # n_fft / 2 < length: the STFT's reflect padding
MAX_SAMPLES = SAMPLE_RATE * handlers.SEG_SECONDS    # one segment of the handlers' loop
MIN_SCORED_SAMPLES = models.MIN_SCORED_SAMPLES
HOP = 441
WINDOW_BATCHES = 8   # the lines of a list are read and restored `WINDOW_BATCHES * max_batch` at a time (host memory of a large set)


def _probe(path):
    """(samples, True) of a 44.1 kHz wav file the handlers' reader takes; (None, False) for anything else (the handler's to judge)."""
    try:
        with wave.open(path, "rb") as f:
            ok = f.getframerate() == SAMPLE_RATE and f.getsampwidth() in (1, 2, 4) and f.getnchannels() >= 1
            return (f.getnframes(), True) if ok else (None, False)
    except (OSError, EOFError, wave.Error):
        return None, False


def is_batched(source, target):
    """The routing rule of `inference` (module docstring) for one list line; target None: a line without a target."""
    n, ok = _probe(source)
    if not ok or not MIN_SAMPLES <= n <= MAX_SAMPLES:
        return False
    if target is None:
        return True
    m, ok = _probe(target)
    return ok and MIN_SAMPLES <= m <= MAX_SAMPLES and m >= MIN_SCORED_SAMPLES and m // HOP == n // HOP


def _handler_of(model):
    return handlers.handler_ssr_unet if isinstance(model, models.SSR_UNet) else handlers.handler_gsr_voicefixer


def _run_handler(handler, model, source, output, target, meta):
    """One per-file handler call on `model` (the handlers keep their model in handlers._state)."""
    saved = dict(handlers._state)
    handlers._state["model"] = model
    try:
        return handler(input=source, output=output, target=target, ckpt=None, device=model.device, needrefresh=False, meta=meta)
    finally:
        handlers._state.clear()
        handlers._state.update(saved)


def _restore_window(model, lines, unify, max_batch):
    """The batched lines of one window -> {position in `lines`: (restored clip, scores)}.  A file whose data chunk is shorter than
    its header promised no longer meets the rule it was admitted by: it is left to the handler."""
    scored, plain = [], []
    for k, (source, target) in enumerate(lines):
        if not is_batched(source, target):
            continue
        x = handlers.load_wav(source, SAMPLE_RATE)
        t = handlers.load_wav(target, SAMPLE_RATE) if target is not None else None
        if x.shape[0] != _probe(source)[0] or (t is not None and t.shape[0] != _probe(target)[0]):
            continue
        (scored if t is not None else plain).append((k, x, t))
    done = {}
    if scored:
        kw = {"max_batch": max_batch}
        if "unify_energy" in inspect.signature(model.restore_scored_list).parameters:
            kw["unify_energy"] = unify
        wavs, scores = model.restore_scored_list([clips.as_tensor(x) for _, x, _ in scored], [clips.as_tensor(t) for _, _, t in scored], **kw)
        for (k, _, _), w, s in zip(scored, wavs, scores):
            done[k] = (w, s)
    if plain:
        kw = {"max_batch": max_batch}
        if "unify_energy" in inspect.signature(model.restore_list).parameters:
            kw["unify_energy"] = unify
        for (k, _, _), w in zip(plain, model.restore_list([clips.as_tensor(x) for _, x, _ in plain], **kw)):
            done[k] = (w, {})
    return done


def inference(model, save_dir, testsets, metas, limit_number=None, max_batch=128, handler=None):
    """evaluation_proc/eval.py:89-135 for `model` (a models.VoiceFixer or SSR_UNet with its weights loaded).  metas[testset] =
    {"rate", "list": path of the `source [target]` list, "unify_energy": optional} -- the dict metrics.aggregate_score takes, plus
    the handler's switch.  Writes save_dir/testset/basename(source) and the .json beside it for every line, in list order; which
    files are batched: the module docstring.  handler: the per-file fallback (default: the model's own handler)."""
    handler = handler or _handler_of(model)
    for n, testset in enumerate(testsets):
        logging.info("restoring %s (%d / %d)", testset, n + 1, len(testsets))
        res_dir = os.path.join(save_dir, testset)
        os.makedirs(res_dir, exist_ok=True)
        meta = metas[testset]
        lst = metrics.read_list(meta["list"])
        if limit_number is not None:
            lst = lst[:limit_number]
        lines = [metrics._parse(line) for line in lst]
        unify = bool(meta.get("unify_energy", False))
        step = max(1, WINDOW_BATCHES * int(max_batch))
        for a in range(0, len(lines), step):
            window = lines[a:a + step]
            done = _restore_window(model, window, unify, max_batch)
            for k, (source, target) in enumerate(window):      # list order: a basename that occurs twice keeps its last line's files
                output = os.path.join(res_dir, os.path.basename(source))
                if k in done:
                    wav, scores = done[k]
                    handlers.save_wave(clips.as_numpy(wav), output, SAMPLE_RATE)
                else:
                    scores = _run_handler(handler, model, source, output, target, meta)
                metrics.write_json(scores, output[:-4] + ".json")


def evaluation(output_path, model, description, testsets, metas, limit_phrase_number=None, stoi=False, bsseval=False):
    """evaluation_proc/eval.py:142-221: `inference` into output_path/<date>_<description>_<id>, metrics.aggregate_score per test set
    (on the model's engine; stoi=True adds STOI, bsseval=True the BSS Eval sdr, isr, sar), metrics.gather_score.  Returns that
    directory."""
    run = time.strftime("%Y-%m-%d", time.localtime()) + "_" + description + "_" + str(int(random.random() * 1000))
    output_path = os.path.join(output_path, run)
    inference(model, output_path, testsets, metas, limit_number=limit_phrase_number)
    for testset in testsets:
        try:
            metrics.aggregate_score(output_path, [testset], limit_number=limit_phrase_number, metas=metas,
                                    engine=getattr(model, "engine", None), stoi=stoi, bsseval=bsseval)
        except Exception as e:      # (the reference logs a test set that fails to score and goes on to the next)
            logging.exception(e)
    metrics.gather_score(output_path, testsets)
    return output_path
