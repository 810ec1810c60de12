"""Scoring of restored test sets: the drop-in for evaluation_proc.metrics.AudioMetrics and eval.py's aggregate_score / gather_score.

`AudioMetrics.evaluation` (evaluation_proc/metrics.py:55-81) returns these keys, computed on the GPU by vfx_audio_metrics_rate
(include/vfx.h; Engine.audio_metrics) with the front end the reference picks from the target's sample rate
(evaluation_proc/metrics.py:37-51): n_fft 2048, hop 441 and 128 mel bands at 44.1 kHz; n_fft 743, hop 160 and 80 mel bands at 16 kHz
(an odd n_fft: 371 samples of reflect padding on each side, 1 + (n - 1) // 160 frames):

    sisdr, lsd, non_log_sispec, sispec, ssim, final_mel_lsd, final_non_log_mel_sispec, final_mel_sispec, final_mel_ssim

and, with `stoi=True`, the key `stoi` right after `sisdr` (the reference's order), computed on the GPU by vfx_stoi (Engine.stoi) from
the same padded batches.  STOI is restated from the published algorithm (Taal, Hendriks, Heusdens, Jensen 2011; the authors' MATLAB;
pystoi's stoi(extended=False): 10 kHz by Octave's resample filter, frames at range(0, n - 256, 128) -- the last aligned frame is not
taken --, 1e-5 for fewer than 30 frames) and, like SI-SDR, held against a float64 restatement (tests/stoi_f64.py: within 1e-9), not
pinned against the pystoi package.

With `bsseval=True` the keys `sdr`, `isr`, `sar` follow the others: BSS Eval v4 "images" (Vincent, Gribonval, Fevotte 2006; the
SiSEC 2018 form speechmetrics calls with window = inf) for one source, one channel and one window over the whole file, with a 512-tap
distortion filter, computed on the GPU by vfx_bsseval (Engine.bsseval) from the same padded batches.  They are restated from the
definition in include/vfx.h and held against a float64 restatement (tests/bsseval_f64.py: within 1e-9 dB), not pinned against the
museval package.  A silent est or target scores NaN in all three (museval's rule), which the mean row skips as pandas does.

What differs from the reference, on purpose:
  * STOI and the bsseval scores are opt-in (`stoi=True`, `bsseval=True`) and restated; PESQ is not computed, and its key is absent
    (no implementation to pin it against).
  * 44.1 kHz and 16 kHz targets (the rates in the engine's `score_rates`; an engine without that attribute scores 44.1 kHz only): any
    other rate raises ValueError, like the reference's "Bad Samplerate" for rates it has no STFT for.  An est file at another rate
    than its target, or of another length, makes that pair an error: speechmetrics would zero-pad the shorter signal and
    librosa.load would resample est.
  * aggregate_score leaves a pair that fails out of the table and its mean; the reference records the previous pair's scores
    under the failed pair's name again.
"""
import csv
import json
import logging
import os
import wave

import numpy as np
import torch

from . import handlers

METRIC_KEYS = ("sisdr", "lsd", "non_log_sispec", "sispec", "ssim",
               "final_mel_lsd", "final_non_log_mel_sispec", "final_mel_sispec", "final_mel_ssim")
BSSEVAL_KEYS = ("sdr", "isr", "sar")
SAMPLE_RATE = 44100
MIN_SAMPLES = 6 * 441   # 7 STFT frames: skimage's 7 x 7 SSIM rejects a smaller spectrogram
# rate -> (hop, fewest samples that give 7 STFT frames): T = n // 441 + 1 at n_fft 2048; T = 1 + (n - 1) // 160 at the odd n_fft 743
FRONT_ENDS = {SAMPLE_RATE: (441, MIN_SAMPLES), 16000: (160, 6 * 160 + 1)}


def read_list(fname):
    """evaluation_proc/utils.py:73-79."""
    with open(fname, "r") as f:
        return [line.strip("\n") for line in f.readlines()]


def write_json(d, fname):
    with open(fname, "w") as f:
        f.write(json.dumps(d))


def load_json(fname):
    with open(fname, "r") as f:
        return json.load(f)


def _wav_info(path):
    with wave.open(path, "rb") as f:
        return f.getnframes(), f.getframerate()


class AudioMetrics:
    """evaluation_proc/metrics.py:20-106 at 44.1 kHz or 16 kHz.  `engine`: an Engine (or anything with `device` and
    `audio_metrics(est, target, lengths)` -- and, for `stoi=True`, `stoi(est, target, lengths, fs)`, for `bsseval=True`,
    `bsseval(est, target, lengths)`); default: a new Engine on cuda:0.
    A rate other than 44100 must be in the engine's `score_rates`, and is handed to it as `audio_metrics(..., rate=rate)`.
    stoi=True adds the key "stoi" after "sisdr"; bsseval=True appends BSSEVAL_KEYS."""

    def __init__(self, rate, engine=None, stoi=False, bsseval=False):
        if engine is None and int(rate) in FRONT_ENDS:
            from .engine import Engine
            engine = Engine("cuda:0")
        rates = (SAMPLE_RATE,) + tuple(getattr(engine, "score_rates", ()))
        if int(rate) not in rates or int(rate) not in FRONT_ENDS:
            raise ValueError("Bad Samplerate: %s (test sets at %s Hz are scored)" % (rate, " or ".join(str(r) for r in sorted(set(rates)))))
        self.rate = int(rate)
        self.hop, self.min_samples = FRONT_ENDS[self.rate]
        self.engine = engine
        self.stoi = bool(stoi)
        self.bsseval = bool(bsseval)
        self.keys = METRIC_KEYS[:1] + ("stoi",) + METRIC_KEYS[1:] if self.stoi else METRIC_KEYS
        if self.bsseval:
            self.keys = self.keys + BSSEVAL_KEYS

    # ------------------------------------------------------------------ files
    def evaluation(self, est, target):
        """est, target: .wav paths -> {key: float} (self.keys: METRIC_KEYS, with "stoi" second and BSSEVAL_KEYS last when asked for); {} when
        target is None."""
        if target is None:
            return {}
        r = self.evaluation_list([(est, target)])[0]
        if isinstance(r, Exception):
            raise r
        return r

    def _check_pair(self, est, target):
        (n_e, sr_e), (n_t, sr_t) = _wav_info(est), _wav_info(target)
        if sr_t != self.rate:
            raise ValueError("Bad Samplerate: %s is at %d Hz, the test set at %d Hz" % (target, sr_t, self.rate))
        if sr_e != sr_t:
            raise ValueError("%s is at %d Hz, its target %s at %d Hz" % (est, sr_e, target, sr_t))
        if n_e != n_t:
            raise ValueError("%s has %d samples, its target %s %d" % (est, n_e, target, n_t))
        if n_t < self.min_samples:
            raise ValueError("%s has %d samples: SSIM needs at least %d (7 STFT frames)" % (target, n_t, self.min_samples))
        return n_t

    def evaluation_list(self, pairs, max_batch=128):
        """[(est_path, target_path), ...] -> one entry per pair, in order: the {key: float} dict, or the exception that pair
        raised.  The pairs are read and scored sorted by length, up to `max_batch` per padded batch (one vfx_audio_metrics call and,
        with stoi, one vfx_stoi call, with bsseval, one vfx_bsseval call on the same device tensors)."""
        results = [None] * len(pairs)
        ok = []
        for i, (est, target) in enumerate(pairs):
            try:
                ok.append((self._check_pair(est, target), i))
            except Exception as e:  # noqa: BLE001 -- reported per pair
                results[i] = e
        ok.sort()
        dev = getattr(self.engine, "device", torch.device("cpu"))
        for at in range(0, len(ok), max_batch):
            chunk = ok[at:at + max_batch]
            Lmax = chunk[-1][0]
            est = np.zeros((len(chunk), Lmax), np.float32)
            tgt = np.zeros((len(chunk), Lmax), np.float32)
            lengths, idx = [], []
            for j, (n, i) in enumerate(chunk):
                try:
                    e = handlers.load_wav(pairs[i][0], self.rate)
                    t = handlers.load_wav(pairs[i][1], self.rate)
                except Exception as ex:  # noqa: BLE001
                    results[i] = ex
                    continue
                est[len(idx), :n], tgt[len(idx), :n] = e, t
                lengths.append(n)
                idx.append(i)
            if not idx:
                continue
            k = len(idx)
            e_dev, t_dev = torch.from_numpy(est[:k]).to(dev), torch.from_numpy(tgt[:k]).to(dev)
            if self.rate == SAMPLE_RATE:   # (three arguments: what an engine without `score_rates` takes)
                scores = self.engine.audio_metrics(e_dev, t_dev, lengths)
            else:
                scores = self.engine.audio_metrics(e_dev, t_dev, lengths, rate=self.rate)
            scores = scores.cpu().numpy().tolist()
            if self.stoi:
                st = self.engine.stoi(e_dev, t_dev, lengths, fs=self.rate).cpu().numpy().tolist()
                scores = [row[:1] + [st[j]] + row[1:] for j, row in enumerate(scores)]
            if self.bsseval:
                bs = self.engine.bsseval(e_dev, t_dev, lengths).cpu().numpy().tolist()
                scores = [row + bs[j] for j, row in enumerate(scores)]
            for j, i in enumerate(idx):
                results[i] = {key: float(v) for key, v in zip(self.keys, scores[j])}
        return results

    # ------------------------------------------------------------------ tensors (metrics.py:83-106)
    def lsd(self, est, target):
        """(B, C, T, F) linear magnitudes -> (B, C, 1, 1)."""
        return handlers.lsd(est, target)

    def sispec(self, est, target):
        """(B, C, T, F) -> the batch mean, a 0-d tensor."""
        return handlers.sispec(est, target)

    def ssim(self, est, target):
        """(B, C, T, F) -> (B, C, 1, 1) float64: skimage structural_similarity(win_size=7) per (batch, channel) image."""
        if est.shape[-1] < 7 or est.shape[-2] < 7:
            raise ValueError("ssim: an image of %s is smaller than the 7 x 7 window" % (tuple(est.shape[-2:]),))
        return handlers.ssim(est, target)


def _parse(line):
    parts = line.split(" ")
    return (parts[0], None) if len(parts) == 1 else (parts[0], parts[1])


def _means(rows):
    """Column means over the rows that hold a number in that column (pandas DataFrame.mean); a NaN in a BSSEVAL_KEYS column -- a
    silent est or target -- is skipped like a missing value, as pandas does."""
    cols, sums, counts = [], {}, {}
    for r in rows.values():
        for k, v in r.items():
            if k not in sums:
                cols.append(k)
                sums[k], counts[k] = 0.0, 0
            if isinstance(v, (int, float)) and not isinstance(v, bool) and not (k in BSSEVAL_KEYS and v != v):
                sums[k] += float(v)
                counts[k] += 1
    return cols, {k: (sums[k] / counts[k] if counts[k] else float("nan")) for k in cols}


def _write_table(path, rows, cols, mean_row=None):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + cols)
        for name, r in rows.items():
            w.writerow([name] + [repr(r[c]) if isinstance(r.get(c), float) else r.get(c, "") for c in cols])
        if mean_row is not None:
            w.writerow(["mean"] + [repr(mean_row[c]) for c in cols])


def aggregate_score(save_dir, testsets, limit_number=None, metas=None, engine=None, stoi=False, bsseval=False):
    """evaluation_proc/eval.py:25-86.  metas[testset] = {"rate": ..., "list": path of the `source [target]` list}; the restored
    file of a line is save_dir/testset/basename(source).  Per pair with a target: the scores, updated with the handler's JSON
    beside the restored file (save_dir/testset/<name>.json, when it exists), are written back to that JSON.  Per test set:
    <testset>.csv (one row per target basename and a `mean` row) and result.json (the means).  A pair that fails is logged and
    left out.  stoi=True: the scores carry "stoi" (AudioMetrics(stoi=True)), and so do the tables and means; bsseval=True: likewise
    "sdr", "isr", "sar" (AudioMetrics(bsseval=True)).  Returns {testset: {target basename: scores}}."""
    if metas is None:
        raise ValueError("aggregate_score: metas ({testset: {'rate', 'list'}}) is required (the reference's Config is not part of "
                         "this package)")
    result = {}
    for n, testset in enumerate(testsets):
        logging.info("scoring %s (%d / %d)", testset, n + 1, len(testsets))
        res_dir = os.path.join(save_dir, testset)
        os.makedirs(res_dir, exist_ok=True)
        meta = metas[testset]
        lst = read_list(meta["list"])
        if limit_number is not None:
            lst = lst[:limit_number]
        judger = AudioMetrics(rate=meta["rate"], engine=engine, stoi=stoi, bsseval=bsseval)
        pairs, names = [], []
        for line in lst:
            source, target = _parse(line)
            if target is None:
                continue
            pairs.append((os.path.join(res_dir, os.path.basename(source)), target))
            names.append(os.path.basename(target))
        rows = {}
        for (est, target), name, r in zip(pairs, names, judger.evaluation_list(pairs)):
            if isinstance(r, Exception):
                logging.error("scoring %s against %s failed: %r", est, target, r)
                continue
            js = est[:-4] + ".json"
            if os.path.exists(js):
                r.update(load_json(js))
            write_json(r, js)
            rows[name] = r
        result[testset] = rows
        if pairs:
            cols, mean = _means(rows)
            _write_table(os.path.join(res_dir, testset + ".csv"), rows, cols, mean)
            write_json(mean, os.path.join(res_dir, "result.json"))
            logging.info("%s: %s", testset, mean)
    return result


def gather_score(output_path, testsets):
    """evaluation_proc/eval.py:224-230: output_path/result.csv, one row per test set that has a result.json."""
    final = {}
    for t in testsets:
        p = os.path.join(output_path, t, "result.json")
        if os.path.exists(p):
            final[t] = load_json(p)
    if final:
        cols, _ = _means(final)
        _write_table(os.path.join(output_path, "result.csv"), final, cols)
    return final
