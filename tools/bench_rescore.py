"""Rescoring of a lattice's sentences, `AttentionDecoderTCN.score_sentences`: the device path (prefix
trie, one label step per trie level, DeviceForcedScorer) against the per-sentence host loop
(ASR_FORCED_NATIVE=0) on the same device (development tool; bench.py is the contract benchmark).

Decoder dimensions of egs/wsj/yamls/lattice_decoding/tcn.yaml (tcn_hidden_size 384, att_hidden_size
64, dilations [1, 2], 2 layers per block, temperature 1.25), random weights, a random encoder output
of 334 frames, the shipped trigram character LM started behind its epsilon arc (`closed_start` of
tools/bench_lm_decode.py, so the bags are not empty), the scripts' settings (lm_weight 0.8,
coverage 0.5 / 0.1, length_normalization 1.2).

Sentence sets, seeded and lattice-like: a base sentence of --length labels and N variants of it that
each change one to three positions, every position drawing from three alternatives of its own; N in
--sentences (default 1 64 512), one utterance per call.  The ground-truth shape of
score_groundtruth.py: --utterances (default 16) utterances with one sentence each, one call.

Both paths are warmed up, then timed alternately --iters times; a timed window repeats the call until
it lasts about half a second.  The host path at more than --host-cap (default 64) sentences is timed
on the first --host-subset (default 32) of them and scaled by N / 32 (said in the output and the JSON:
`scaled`).
Reported besides: the units (distinct prefixes) the device path runs against sentences x positions,
the work the trie saves, and the largest difference of a loss between the two paths on the sentences
the host path scored.  --out writes the JSON (profiles/r13_rescore.json)."""
import argparse
import datetime
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-asr_amd'))

from att_speech.lm_fst import LmFst                      # noqa: E402
from att_speech.modules.beam_search import sentence_trie  # noqa: E402
from att_speech.modules.tcn import AttentionDecoderTCN   # noqa: E402
from bench_lm_decode import closed_start, lm_vocabulary  # noqa: E402

SWITCH = 'ASR_FORCED_NATIVE'


def lattice_like(rng, letters, length, n):
    """base + variants changing 1..3 positions, each position with 3 alternatives of its own"""
    base = [int(c) for c in rng.choice(letters, size=length)]
    alternatives = rng.choice(letters, size=(length, 3))
    out = [base]
    for _ in range(n - 1):
        s = list(base)
        for pos in rng.choice(length, size=int(rng.integers(1, 4)), replace=False):
            s[int(pos)] = int(alternatives[int(pos), int(rng.integers(0, 3))])
        out.append(s)
    return out[:n]


def window(fn, seconds):
    """one timed window: `fn` repeated until about `seconds` have passed -> seconds per call"""
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    reps = max(1, int(math.ceil(seconds / max(first, 1e-6))) - 1)
    if reps == 1 and first >= seconds:
        return first
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(dec, enc, lens, sentences, a, name):
    total = sum(len(s) for s in sentences)
    positions = sum(len(x) + 1 for s in sentences for x in s)
    cap = a.host_cap
    scaled = len(sentences) == 1 and total > cap
    host_sentences = [sentences[0][:a.host_subset]] if scaled else sentences
    host_total = sum(len(s) for s in host_sentences)

    def native():
        os.environ[SWITCH] = '1'
        return dec.score_sentences(enc, lens, sentences)

    def host():
        os.environ[SWITCH] = '0'
        return dec.score_sentences(enc, lens, host_sentences)
    got, want = native(), host()                                   # warm-up of both, and the check
    units = sum(lv['n_units'] for s in sentences for lv in sentence_trie(s, dec.EOS)['levels'])
    diff = 0.0
    for g, w in zip(got, want):                 # (a sentence the LM cannot read scores -inf on both paths)
        ok = np.isfinite(w['loss'])
        assert (np.isfinite(g['loss'][:len(ok)]) == ok).all()
        diff = max([diff] + np.abs(g['loss'][:len(ok)][ok] - w['loss'][ok]).tolist())
    finite = float(np.mean(np.concatenate([np.isfinite(g['lm']) for g in got])))   # the LM reads most
    same_counts = all(bool((g['covered'][:len(w['covered'])] == w['covered']).all()) for g, w in zip(got, want))
    tn, th = [], []
    for _ in range(a.iters):                                       # alternating
        tn.append(window(native, a.window))
        th.append(window(host, a.window) * total / host_total)
    del os.environ[SWITCH]
    tn, th = sorted(tn), sorted(th)
    res = dict(name=name, utterances=len(sentences), sentences=total, positions=positions, units=units,
               unit_share=units / positions,
               native_ms=dict(median=1e3 * tn[len(tn) // 2], min=1e3 * tn[0], max=1e3 * tn[-1]),
               host_ms=dict(median=1e3 * th[len(th) // 2], min=1e3 * th[0], max=1e3 * th[-1]),
               host_sentences_timed=host_total, scaled=scaled,
               host_over_native=th[len(th) // 2] / tn[len(tn) // 2], max_loss_difference=diff,
               covered_counts_equal=same_counts, lm_finite_share=finite,
               windows=a.iters)
    print('%-14s %4d sentences: native %9.1f ms (%.1f-%.1f), host %10.1f ms (%.1f-%.1f)%s, host/native %.2f; '
          '%d units for %d sentence positions (%.1f %%); largest loss difference %.2g' % (
              name, total, res['native_ms']['median'], res['native_ms']['min'], res['native_ms']['max'],
              res['host_ms']['median'], res['host_ms']['min'], res['host_ms']['max'],
              ' [timed on %d sentences, scaled]' % host_total if scaled else '',
              res['host_over_native'], units, positions, 100.0 * units / positions, diff), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sentences', type=int, nargs='+', default=[1, 64, 512])
    ap.add_argument('--utterances', type=int, default=16)
    ap.add_argument('--length', type=int, default=60)
    ap.add_argument('--frames', type=int, default=334)
    ap.add_argument('--encoded', type=int, default=320)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--host-cap', type=int, default=64)
    ap.add_argument('--host-subset', type=int, default=32)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lm = closed_start(LmFst.read(os.path.join(ROOT, 'tests', 'golden', 'G_char_tg_syms.fst.gz')))
    vocab = lm_vocabulary(lm)
    # labels from the letters, the space and the apostrophe: nearly every such sequence has a finite LM cost
    letters = np.array([k for k, s in enumerate(vocab) if len(s) == 1 and (s.isalpha() or s in " '")])
    torch.manual_seed(0)
    dec = AttentionDecoderTCN(
        {'features': torch.zeros(a.frames, 2, a.encoded)}, len(vocab), tcn_hidden_size=384,
        att_hidden_size=64, dropout_p=0.3, kernel_size=3, dilation_sizes=[1, 2], tcn_layers_per_block=2,
        attention_temperature=1.25, beam_size=1, length_normalization=1.2, vocabulary=vocab, lm_file=lm,
        lm_weight=0.8, coverage_weight=0.5, coverage_tau=0.1).eval().to(dev)
    enc = torch.randn(a.frames, a.utterances, a.encoded, generator=torch.Generator().manual_seed(1)).to(dev)
    res = {'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0),
           'frames': a.frames, 'sentence_length': a.length, 'classes': len(vocab) + 1,
           'lm': 'G_char_tg_syms.fst.gz (closed_start)', 'lm_weight': 0.8, 'coverage_weight': 0.5,
           'coverage_tau': 0.1, 'length_normalization': 1.2, 'window_seconds': a.window, 'cases': []}
    rng = np.random.default_rng(0)
    one = enc[:, :1].contiguous()
    for n in a.sentences:
        res['cases'].append(measure(dec, one, torch.tensor([a.frames]),
                                    [lattice_like(rng, letters, a.length, n)], a, 'lattice N=%d' % n))
    truth = [[[int(c) for c in rng.choice(letters, size=a.length)]] for _ in range(a.utterances)]
    res['cases'].append(measure(dec, enc, torch.full((a.utterances,), a.frames), truth, a,
                                'ground truth'))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
