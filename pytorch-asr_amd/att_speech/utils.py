"""att_speech.utils — the registry functions of the reference (att_speech/utils.py:73-97):
YAML `class_name` -> object; and its evaluation surface (utils.py:35-70, 100-161, 202-218,
221-374): edit distance with operation counts, running statistics, `LogitsDumper`, and
`do_evaluate` with `evaluate_greedy` / `evaluate_greedy_in_train_mode`.

The reference scores every utterance twice (characters, words) with a Python double loop and an
`np.argmin` per cell.  Here `do_evaluate` scores a whole batch, characters and words, with one
launch of `asr_edit_distance_stats_i32` (`score_pairs`, csrc/edit_distance.hip) when the model is
on the GPU, and with a host implementation that sweeps anti-diagonals as numpy vectors otherwise
(`ASR_NATIVE_SCORING=0` forces the host; read per call)."""
from __future__ import absolute_import, division, print_function

import importlib
import os
import warnings
from collections import defaultdict

import numpy as np


def get_class(str_or_class, default_mod=None):
    """`'pkg.module.Name'` -> the object; a bare `'Name'` is looked up in `default_mod`;
    anything that is not a string is returned as it is."""
    if not isinstance(str_or_class, str):
        return str_or_class
    module_path, _, attribute = str_or_class.rpartition('.')
    module_path = module_path or default_mod
    if not module_path:
        raise ValueError('Specify a module for %s' % (str_or_class,))
    return getattr(importlib.import_module(module_path), attribute)


def contruct_from_kwargs(object_kwargs, default_mod=None,
                         additional_parameters=None):
    """Instantiate `object_kwargs['class_name']` with the remaining entries as keyword
    arguments; `additional_parameters` are added last (they win).  The name keeps the
    reference's spelling because callers import it."""
    kwargs = {k: v for k, v in dict(object_kwargs).items() if k != 'class_name'}
    kwargs.update(additional_parameters or {})
    return get_class(object_kwargs['class_name'], default_mod)(**kwargs)


def edit_distance(x, y):
    """Levenshtein distance between two sequences (reference utils.py:18-33)."""
    prev = list(range(len(y) + 1))
    for i, xi in enumerate(x, 1):
        cur = [i]
        for j, yj in enumerate(y, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (xi != yj)))
        prev = cur
    return prev[-1]


def get_mask(lengths, mask_length=None, batch_first=True):
    """1 inside each sequence, 0 on padding (reference utils.py:436-448);
    always on the CPU like `lengths`."""
    import torch
    lengths = torch.as_tensor(lengths)
    if mask_length is None:
        mask_length = int(lengths.max())
    lengths = lengths.long()
    if batch_first:
        mask = torch.arange(mask_length) < lengths[:, None]
    else:
        mask = torch.arange(mask_length)[:, None] < lengths
    return mask.float()


# ---------------------------------------------------------------------------------------------
# scoring: edit distance with operation counts

_FIELD = 21                                   # host cells: dist | ins << 21 | del << 42 in one int64
_FMASK = (1 << _FIELD) - 1
_STEP_INS = 1 | (1 << _FIELD)
_STEP_DEL = 1 | (1 << (2 * _FIELD))
_SCORING_WARNED = {}


def _stats_of_ids(xa, ya):
    """(dist, ins, del, sub) for two integer arrays: the reference's recurrence (utils.py:44-53),
    the first minimum winning in the order up ("ins"), left ("del"), diagonal ("sub"), with the
    counts of its trace-back (utils.py:54-64) carried forward from the chosen predecessor: a
    move adds to its count only where the distance grows, so dist == ins + del + sub and `sub`
    needs no field.  The cells of one anti-diagonal do not depend on each other; each is one numpy
    expression over the two diagonals before it."""
    n, m = len(xa), len(ya)
    if n == 0:
        return m, 0, m, 0
    if m == 0:
        return n, n, 0, 0
    if max(n, m) > _FMASK:
        raise ValueError('edit_distance_with_stats: sequences longer than %d' % _FMASK)
    idx = np.arange(max(n, m) + 1, dtype=np.int64)
    col0, row0 = idx * _STEP_INS, idx * _STEP_DEL          # cell(i, 0): all "ins"; cell(0, j): all "del"
    yr = ya[::-1]
    # d2[i], d1[i] = cell(i, d - 2 - i), cell(i, d - 1 - i): the two diagonals before diagonal d
    d2, d1, new = (np.zeros(n + 1, np.int64) for _ in range(3))
    d1[0], d1[1] = row0[1], col0[1]
    for d in range(2, n + m + 1):
        lo, hi = max(1, d - m), min(n, d - 1)
        up, left, diag = d1[lo - 1:hi], d1[lo:hi + 1], d2[lo - 1:hi]
        neq = (xa[lo - 1:hi] != yr[m - d + lo:m - d + hi + 1]).astype(np.int64)
        cu, cl, cd = (up & _FMASK) + 1, (left & _FMASK) + 1, (diag & _FMASK) + neq
        new[lo:hi + 1] = np.where((cu <= cl) & (cu <= cd), up + _STEP_INS,
                                  np.where(cl <= cd, left + _STEP_DEL, diag + neq))
        if d <= m:
            new[0] = row0[d]
        if d <= n:
            new[d] = col0[d]
        d2, d1, new = d1, new, d2
    v = int(d1[n])
    dist, ins, dele = v & _FMASK, (v >> _FIELD) & _FMASK, v >> (2 * _FIELD)
    return dist, ins, dele, dist - ins - dele


def _token_ids(seqs):
    """Every token of `seqs` (sequences of hashables) as an integer, through one dict: exact for
    any vocabulary."""
    table = {}
    return [[table.setdefault(tok, len(table)) for tok in seq] for seq in seqs]


def edit_distance_with_stats(x, y):
    """(reference utils.py:35-65) -> (dist, {'ins', 'del', 'sub'}) for hypothesis x against
    reference text y, any sequences of hashables."""
    xa, ya = _token_ids([x, y])
    dist, ins, dele, sub = _stats_of_ids(np.asarray(xa, np.int64), np.asarray(ya, np.int64))
    return dist, {'ins': ins, 'del': dele, 'sub': sub}


def word_error_rate(x, y):
    """Edit distance between x and y as a fraction of len(x) (reference utils.py:68-70: the first
    argument is the one the rate is relative to)."""
    return float(edit_distance(x, y)) / len(x)


def _score_pairs_host(ids, n):
    out = np.empty((n, 4), np.int64)
    for p in range(n):
        out[p] = _stats_of_ids(np.asarray(ids[p], np.int64), np.asarray(ids[n + p], np.int64))
    return out


def _score_pairs_device(ids, n, device):
    """One launch of asr_edit_distance_stats_i32 over all pairs -> int32 [n, 4] on `device`, or
    None (after one warning) when a side is longer than the kernel is built for.  One pinned
    buffer and one asynchronous copy carry offsets and tokens; nothing waits for the device."""
    import torch
    from att_speech import _native
    lens = np.fromiter((len(s) for s in ids), np.int64, 2 * n)
    max_x, max_y = (int(lens[:n].max()), int(lens[n:].max())) if n else (0, 0)
    limit = _native.edit_distance_max_len()
    if max(max_x, max_y) > limit:
        if not _SCORING_WARNED.get('limit'):
            _SCORING_WARNED['limit'] = True
            warnings.warn('score_pairs: a sequence of %d tokens exceeds the %d the native edit-distance '
                          'kernel is built for; such batches are scored on the host'
                          % (max(max_x, max_y), limit))
        return None
    nx, ny = int(lens[:n].sum()), int(lens[n:].sum())
    buf = np.zeros(2 * (n + 1) + nx + ny, np.int32)
    np.cumsum(lens[:n], out=buf[1:n + 1])
    np.cumsum(lens[n:], out=buf[n + 2:2 * n + 2])
    buf[2 * n + 2:] = [t for s in ids for t in s]
    dev = torch.from_numpy(buf).pin_memory().to(device, non_blocking=True)
    tok = dev[2 * n + 2:]
    return _native.edit_distance_stats(tok[:nx], dev[:n + 1], tok[nx:], dev[n + 1:2 * n + 2],
                                       max_x, max_y)


def _native_scoring(device):
    if device is None or os.environ.get('ASR_NATIVE_SCORING', '1') == '0':
        return False
    import torch
    from att_speech import _native
    return torch.device(device).type == 'cuda' and os.path.exists(_native.LIB_PATH)


def _score_pairs(hyps, refs, device):
    """-> int32 [n, 4] tensor on `device` (native) or int64 numpy array [n, 4] (host)"""
    hyps, refs = list(hyps), list(refs)
    if len(hyps) != len(refs):
        raise ValueError('score_pairs: %d hypotheses against %d references' % (len(hyps), len(refs)))
    ids = _token_ids(hyps + refs)
    out = _score_pairs_device(ids, len(hyps), device) if _native_scoring(device) else None
    return _score_pairs_host(ids, len(hyps)) if out is None else out


def score_pairs(hyps, refs, device=None):
    """edit_distance_with_stats over a batch: `hyps[p]` against `refs[p]`, sequences of any
    hashables -> int64 array [n, 4] of (dist, ins, del, sub).  The tokens of the whole call become
    integers through one dict on the host.  With `device` a GPU all pairs are scored by ONE launch
    of asr_edit_distance_stats_i32; on the CPU, without the library or with ASR_NATIVE_SCORING=0
    (read per call) by the host implementation."""
    out = _score_pairs(hyps, refs, device)
    return out if isinstance(out, np.ndarray) else out.cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------------------------------------
# evaluation bookkeeping

def uniq(inlist):
    """Runs of equal neighbours, like the UNIX `uniq` command (reference utils.py:100-118): the
    (start, end) pairs, in order, for which inlist[start:end] repeats one element.  A one-element
    list gives [(0, 1)] (the reference's loop never binds its counter there and fails)."""
    runs, start = [], 0
    for pos in range(1, len(inlist) + 1):
        if pos == len(inlist) or inlist[pos] != inlist[start]:
            runs.append((start, pos))
            start = pos
    return runs


class RunningStatistics(object):
    """Mean and variance of a stream in one pass (Welford's recurrence, as reference
    utils.py:121-161 applies it: the first sample is the mean; each later sample x moves the mean
    by (x - mean) / count and adds (x - old mean) * (x - new mean) to the sum of squares, the
    products taken in that order so the results are the same floating-point numbers)."""

    def __init__(self):
        super(RunningStatistics, self).__init__()
        self._k, self._m, self._s = 0, 0, 0

    def add(self, data):
        """any array-like of samples (a scalar too), taken in flattened order"""
        for x in np.ravel(data):
            self._k += 1
            if self._k == 1:
                self._m, self._s = x, 0
                continue
            step = float(x - self._m)
            self._m = self._m + step / self._k
            self._s = self._s + step * (x - self._m)

    def mean(self):
        return self._m

    def variance(self):
        """unbiased; 0.0 below two samples"""
        if self._k < 2:
            return 0.0
        return self._s / (self._k - 1)


class LogitsDumper(object):
    """One Kaldi float-matrix archive of decoder logits per evaluation (reference utils.py:202-218):
    `<path>/<num_iter>.ark`, which exists only once complete (it is written as
    `<num_iter>.ark.temp` and renamed by `end`).  `add_batch` takes time-major logits [T, B, C]
    and writes the utterances of the batch in the sorted order of their ids."""

    def __init__(self, path, num_iter):
        os.makedirs(path, exist_ok=True)
        self.end_filename = os.path.join(path, '%s.ark' % (num_iter,))
        self.filename = self.end_filename + '.temp'
        self.owriter = None

    def start(self):
        from att_speech.ctc_forward import KaldiFloatMatrixWriter
        self.owriter = KaldiFloatMatrixWriter('ark:' + self.filename)

    def add_batch(self, uttids, logits):
        per_utt = logits.detach().cpu().numpy().transpose(1, 0, 2)       # [B, T, C]
        for b in np.argsort(uttids):
            self.owriter[uttids[b]] = per_utt[b]

    def end(self):
        self.owriter.close()
        self.owriter = None
        os.rename(self.filename, self.end_filename)


def _read_losses(pending):
    """[(key, loss)] in batch order -> [(key, float)]: what `.item()` gives for each, the device
    tensors read with one copy (widening to float64 is exact)."""
    import torch
    on_dev = [i for i, (_, v) in enumerate(pending) if isinstance(v, torch.Tensor) and v.is_cuda]
    vals = [None] * len(pending)
    if on_dev:
        got = torch.stack([pending[i][1].detach().reshape(()).to(torch.float64) for i in on_dev]).tolist()
        for i, g in zip(on_dev, got):
            vals[i] = g
    for i, (_, v) in enumerate(pending):
        if vals[i] is None:
            vals[i] = v.item() if hasattr(v, 'item') else v
    return [(k, vals[i]) for i, (k, _) in enumerate(pending)]


_BATCH_KEYS_NOT_FOR_DECODE = ('features', 'texts', 'spkids', 'uttids', 'ivectors')
_DATA_LOSS_FIELDS = ('text_loss', 'generated_loss', 'logits_text_diff')
_DATA_LOSS_REQUEST = {'return_texts_and_generated_loss': True, 'return_logits_text_diff': True}


def _print_samples(tokeniser, frames, texts, text_lens, count):
    """`Ref:` / `Decode:` lines for the first `count` utterances: the reference text next to the
    frame-level output, padding shown as a degree sign (what reference utils.py:297-311 prints)."""
    for i, frame_ids in enumerate(frames[:count]):
        shown = ''.join(chr(176) if ch == '<pad>' else ch
                        for ch in tokeniser(frame_ids)[0])
        print('Ref:    ', tokeniser(texts[i][:text_lens[i]])[2])
        print('Decode: ', shown)


def do_evaluate(dataset, model, output_callback=None,
                progress_callback=None, model_in_eval=True,
                generate_data_losses=False, logits_dumper=None,
                print_num_samples=0):
    """Decode every batch of `dataset` with `model` and score it against the transcripts: the
    evaluation of reference utils.py:221-364, with its contract.

    dataset: an iterable of batch dicts whose `.dataset` has
    `ids_to_chars_words_sentence(ids, ignore_noise=)`; every batch key other than features / texts /
    spkids / uttids / ivectors is passed to `model.decode` as a keyword.  `model.decode` returns
    'decoded' (label lists) and 'loss' (a tensor or a dict of tensors), optionally
    'decoded_scores', 'decoded_frames' (printed for the first batch, `print_num_samples` of them)
    and 'logits' (for `logits_dumper`); with `generate_data_losses` it is asked for the
    per-utterance 'text_loss', 'generated_loss' and 'logits_text_diff' too.
    `progress_callback(batch index, number of batches, batch size)` runs before each decode;
    `output_callback` gets one keyword row per utterance: uttid, recognized, original, wer, cer,
    wer_stat, cer_stat, text_loss, other, generated_loss, logits_text_diff.
    Returns {each loss key: its mean over the batches, 'WER', 'CER', 'len_ratio'}.  An empty
    reference text divides by zero, as it does in the reference.

    What differs from the reference is where the time goes: the words and the characters of a
    whole batch are scored by one launch (`score_pairs`), the loss values stay tensors until the
    end and are read once, in batch order (so the running means are the same numbers), and the
    distances are read back per batch only for an `output_callback`; without one they are summed
    on the device and read once.  Nothing here waits for the device per batch beyond what
    `model.decode` does itself."""
    import torch
    model.train(not model_in_eval)
    device = next(model.parameters()).device
    tokeniser = dataset.dataset.ids_to_chars_words_sentence
    n_batches = len(dataset)

    pending_losses = []
    host_dist = np.zeros(2, np.float64)     # summed distances: words, characters
    device_dist = None                      # the same as int64 [2] on the device, while nobody reads them
    ref_len = [0., 0.]                      # reference words, characters
    ratio_sum, n_utts = 0., 0

    if logits_dumper:
        logits_dumper.start()
    for j, batch in enumerate(dataset):
        features, feature_lens = batch['features']
        texts, text_lens = batch['texts']
        ivectors = batch['ivectors']
        if device.type == 'cuda':
            features = features.to(device)
            ivectors = ivectors.to(device) if ivectors is not None else None
        extra = {k: v for k, v in batch.items() if k not in _BATCH_KEYS_NOT_FOR_DECODE}
        if progress_callback:
            progress_callback(j, n_batches, features.size(0))
        positional = (features, feature_lens, batch['spkids'], texts, text_lens)
        if generate_data_losses:      # encoder_args, decoder_args
            positional += ({}, dict(_DATA_LOSS_REQUEST))
        decoded = model.decode(*positional, ivectors=ivectors, **extra)
        per_utt = {f: decoded[f] if generate_data_losses else None for f in _DATA_LOSS_FIELDS}
        if logits_dumper:
            logits_dumper.add_batch(batch['uttids'], decoded['logits'])
        loss = decoded['loss']
        pending_losses += list(loss.items()) if isinstance(loss, dict) else [('loss', loss)]
        if j == 0 and 'decoded_frames' in decoded:
            _print_samples(tokeniser, decoded['decoded_frames'], texts, text_lens, print_num_samples)

        # (chars, words, sentence) per utterance.  The reference hands the tokeniser tensor
        # slices; the same ids as Python integers make its O(L) loop some ten times cheaper (no
        # 0-dim tensor per character)
        rows, lens = texts.tolist(), text_lens.tolist()
        hyp = [tokeniser(ids, ignore_noise=True) for ids in decoded['decoded']]
        ref = [tokeniser(rows[i][:lens[i]], ignore_noise=True) for i in range(len(hyp))]
        nb = len(hyp)
        # one scoring call: pairs [0, nb) are the words, [nb, 2 nb) the characters
        counts = _score_pairs([h[1] for h in hyp] + [h[0] for h in hyp],
                              [r[1] for r in ref] + [r[0] for r in ref], device)
        if not isinstance(counts, np.ndarray) and output_callback:
            counts = counts.cpu().numpy().astype(np.int64)
        if isinstance(counts, np.ndarray):
            host_dist += counts[:, 0].reshape(2, nb).sum(1)
        else:
            sums = counts[:, 0].view(2, nb).sum(1, dtype=torch.int64)
            device_dist = sums if device_dist is None else device_dist + sums

        scores = decoded.get('decoded_scores') or {}
        for i in range(nb):
            n_words, n_chars = len(ref[i][1]), len(ref[i][0])
            if output_callback:
                row = {f: (per_utt[f][i] if generate_data_losses else None) for f in _DATA_LOSS_FIELDS}
                for name, c, n in (('wer', counts[i], n_words), ('cer', counts[nb + i], n_chars)):
                    row[name] = 1.0 * c[0] / n
                    row[name + '_stat'] = {'ins': int(c[1]), 'del': int(c[2]), 'sub': int(c[3])}
                output_callback(uttid=batch['uttids'][i], recognized=hyp[i][2], original=ref[i][2],
                                other={k: v[i] for k, v in scores.items()}, **row)
            ref_len[0] += n_words
            ref_len[1] += n_chars
            ratio_sum += len(hyp[i][0]) / n_chars
            n_utts += 1

    means = defaultdict(RunningStatistics)
    for key, value in _read_losses(pending_losses):
        means[key].add(value)
    if device_dist is not None:
        host_dist += device_dist.tolist()
    if logits_dumper:
        logits_dumper.end()
    summary = {key: stat.mean() for key, stat in means.items()}
    summary.update(WER=host_dist[0] / ref_len[0], CER=host_dist[1] / ref_len[1],
                   len_ratio=ratio_sum / n_utts)
    return summary


def evaluate_greedy(*args, **kwargs):
    """do_evaluate with the model in eval mode (reference utils.py:367-369)"""
    return do_evaluate(*args, **dict(kwargs, model_in_eval=True))


def evaluate_greedy_in_train_mode(*args, **kwargs):
    """do_evaluate with the model in train mode: dropout and batch statistics as in training
    (reference utils.py:372-374)"""
    return do_evaluate(*args, **dict(kwargs, model_in_eval=False))
