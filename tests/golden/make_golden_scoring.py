#!/usr/bin/env python
"""tests/golden/make_golden_scoring.py — regenerates tests/golden/scoring.npz.

Runs ONLY where the reference checkout exists (/root/reference): it imports the reference's own
att_speech.utils under the installed Python with empty stub modules for the absent third-party
packages and records what its functions return.  Data only; nothing of the reference's source
travels.

Records:
  pairs: flat token ids + prefix offsets of every pair (x = hypothesis, y = reference text) and
      the reference's edit_distance_with_stats as [n, 4] = (dist, ins, del, sub): seeded random
      pairs over alphabets of 2, 3, 5 and 47 symbols with lengths 0-70, empty sides, identical
      sequences, pure insertions / deletions, shifted copies, and a handful with a side of
      130-300 (more than one 64-column strip of the kernel; the reference needs ~0.7 s for a
      300 x 300 pair, so these stay few);
  stats: RunningStatistics mean / variance after each chunk of a seeded series; uniq on a crafted
      list;
  eval_json: a whole do_evaluate run of the reference over a stub dataset of three batches in the
      batch-dict layout of SURVEY.md §8b and a stub model whose `decode` returns recorded label
      lists and losses (batch 0: a dict loss; batch 1: `decoded_scores`), with the WSJ dataset's
      ids_to_chars_words_sentence (egs/wsj/data.py:95-98 over kaldi_dataset.py:180-189, the object
      built without its Kaldi constructor; restated below if that import fails) and the 49 WSJ
      symbols of tests/golden/wsj_vocabulary.txt: the inputs, the summary and every
      output_callback row.

Usage:  python tests/golden/make_golden_scoring.py
"""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'

for name in ['pywrapfst', 'torchtext', 'torchtext.vocab', 'kaldi_io', 'tensorboardX']:
    sys.modules[name] = types.ModuleType(name)
sys.modules['torchtext'].vocab = sys.modules['torchtext.vocab']
sys.modules['torchtext.vocab'].Vocab = object
sys.modules['tensorboardX'].SummaryWriter = object
sys.path.insert(0, REF)

import numpy as np          # noqa: E402
import torch                # noqa: E402

warnings.filterwarnings('ignore')

from att_speech import utils as ref_utils      # noqa: E402  (the REFERENCE's module)


def make_pairs():
    rng = np.random.RandomState(20260)
    pairs = []

    def seq(n, a):
        return rng.randint(0, a, size=n).tolist()

    for a in (2, 3, 5, 47):
        for _ in range(70):
            pairs.append((seq(rng.randint(0, 71), a), seq(rng.randint(0, 71), a)))
        for _ in range(8):                               # a reference text with a few edits
            y = seq(rng.randint(1, 71), a)
            x = list(y)
            for _ in range(rng.randint(1, 6)):
                k = rng.randint(0, len(x) + 1)
                op = rng.randint(0, 3)
                if op == 0:
                    x.insert(k, int(rng.randint(0, a)))
                elif op == 1 and x:
                    x.pop(min(k, len(x) - 1))
                elif x:
                    x[min(k, len(x) - 1)] = int(rng.randint(0, a))
            pairs.append((x, y))
    pairs += [([], []), ([], seq(9, 3)), (seq(9, 3), []), ([], seq(64, 2)), (seq(65, 2), [])]
    for n in (1, 7, 63, 64, 65, 70):
        s = seq(n, 5)
        pairs.append((s, list(s)))                       # identical
        pairs.append((s, s[:n // 2]))                    # pure insertions
        pairs.append((s[:n // 2], s))                    # pure deletions
        pairs.append((s[1:] + s[:1], s))                 # shifted copies
        pairs.append(([0] + s, s + [0]))
    pairs += [([1] * 40, [1] * 33), ([0, 1] * 30, [1, 0] * 30)]
    for n, m, a in ((130, 150, 3), (300, 64, 2), (65, 300, 47), (200, 129, 5), (192, 193, 2),
                    (128, 256, 3)):
        pairs.append((seq(n, a), seq(m, a)))
    want = np.zeros((len(pairs), 4), np.int64)
    for p, (x, y) in enumerate(pairs):
        dist, ops = ref_utils.edit_distance_with_stats(x, y)
        want[p] = (int(dist), ops['ins'], ops['del'], ops['sub'])
    lx = [len(x) for x, _ in pairs]
    ly = [len(y) for _, y in pairs]
    return {
        'pairs_x': np.array([t for x, _ in pairs for t in x], np.int32),
        'pairs_x_off': np.concatenate([[0], np.cumsum(lx)]).astype(np.int32),
        'pairs_y': np.array([t for _, y in pairs for t in y], np.int32),
        'pairs_y_off': np.concatenate([[0], np.cumsum(ly)]).astype(np.int32),
        'pairs_want': want,
    }


def make_stats():
    rng = np.random.RandomState(7)
    series = (rng.standard_normal(57) * 3.0 + 11.0).astype(np.float64)
    chunks = [1, 1, 5, 20, 30]
    rs = ref_utils.RunningStatistics()
    empty_variance = float(rs.variance())
    means, variances, pos = [], [], 0
    for c in chunks:
        rs.add(series[pos:pos + c])
        pos += c
        means.append(float(rs.mean()))
        variances.append(float(rs.variance()))
    crafted = [3, 3, 3, 1, 2, 2, 3, 3, 0, 0, 0, 0, 5, 4, 4]
    return {'rs_series': series, 'rs_chunks': np.array(chunks), 'rs_means': np.array(means),
            'rs_variances': np.array(variances), 'rs_empty_variance': np.array(empty_variance),
            'uniq_in': np.array(crafted), 'uniq_out': np.array(ref_utils.uniq(crafted))}


def wsj_dataset(vocab_file):
    """the reference's WSJDataset without its Kaldi constructor, else a restatement of
    egs/wsj/data.py:95-98 and att_speech/data/kaldi_dataset.py:180-189"""
    itos = [line[:-1] for line in open(vocab_file)]
    stoi = {s: i for i, s in enumerate(itos)}
    try:
        from egs.wsj.data import WSJDataset
        ds = WSJDataset.__new__(WSJDataset)
        ds.vocabulary = types.SimpleNamespace(itos=itos, stoi=stoi)
        ds.ids_to_chars_words_sentence([4, 2, 5], ignore_noise=True)
        return ds, 'reference WSJDataset'
    except Exception:
        class Restated(object):
            vocabulary = types.SimpleNamespace(itos=itos, stoi=stoi)

            def ids_to_chars_words_sentence(self, text_ids, ignore_noise=False):
                shown = [itos[int(i)] for i in text_ids]
                if ignore_noise:
                    shown = [c for c in shown if c != '~']
                text = ''.join(shown)
                return shown, text.split(), text
        return Restated(), 'restated'


def make_eval():
    vocab_file = os.path.join(HERE, 'wsj_vocabulary.txt')
    inner, how = wsj_dataset(vocab_file)
    stoi = inner.vocabulary.stoi
    rng = np.random.RandomState(93)
    sentences = [
        ["THE QUICK BROWN FOX", "A ~ NOISY LINE ~", "MR. SMITH'S SHARES ROSE", "NO"],
        ["PRICES FELL SHARPLY", "IT IS -- HE SAID -- OVER", "X"],
        ["ONE TWO THREE FOUR FIVE SIX", "~", "STOCKS AND BONDS"],
    ]
    letters = [stoi[c] for c in "ETAONISRHL '~."]
    batches, recorded = [], []
    for b, sents in enumerate(sentences):
        refs = [[stoi[c] for c in s] for s in sents]
        if b == 2:
            refs[1] = [stoi['~'], stoi['A'], stoi['~']]         # "~" alone would be an empty reference
        hyps = []
        for r in refs:
            h = list(r)
            for _ in range(rng.randint(0, 5)):
                k = rng.randint(0, len(h) + 1)
                op = rng.randint(0, 3)
                if op == 0:
                    h.insert(k, letters[rng.randint(len(letters))])
                elif op == 1 and len(h) > 1:
                    h.pop(min(k, len(h) - 1))
                elif h:
                    h[min(k, len(h) - 1)] = letters[rng.randint(len(letters))]
            hyps.append(h)
        if b == 1:
            hyps[2] = []                                        # an empty hypothesis
        nb, lmax = len(refs), max(len(r) for r in refs)
        texts = np.zeros((nb, lmax), np.int32)
        for i, r in enumerate(refs):
            texts[i, :len(r)] = r
        val = float(np.float32(3.5 + 1.37 * b + rng.rand()))
        rec = {'uttids': ['utt%d_%d' % (b, i) for i in range(nb)], 'texts': texts.tolist(),
               'text_lens': [len(r) for r in refs], 'decoded': hyps,
               'feature_lens': [40 - 3 * i for i in range(nb)]}
        if b == 0:
            rec['loss'] = {'ctc_loss': float(np.float32(val * 0.75)), 'loss': val}
        else:
            rec['loss'] = val
        if b == 1:
            rec['decoded_scores'] = {'att_score': [float(np.float32(-0.5 * i - 0.25)) for i in range(nb)],
                                     'length': [len(h) for h in hyps]}
        recorded.append(rec)
        batches.append({
            'uttids': rec['uttids'], 'spkids': ['spk%d' % i for i in range(nb)],
            'features': (torch.zeros(nb, 40, 2, 1), torch.tensor(rec['feature_lens'], dtype=torch.int32)),
            'texts': (torch.tensor(texts), torch.tensor(rec['text_lens'], dtype=torch.int32)),
            'ivectors': None, 'graph_matrices': ['stub']})

    class Loader(list):
        dataset = inner

    class StubModel(torch.nn.Module):
        def __init__(self):
            super(StubModel, self).__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.calls = 0

        def decode(self, features, feature_lens, speakers, texts=None, text_lens=None,
                   encoder_args=None, decoder_args=None, ivectors=None, **kwargs):
            assert list(kwargs) == ['graph_matrices']
            rec = recorded[self.calls]
            self.calls += 1
            loss = rec['loss']
            loss = ({k: torch.tensor(v, dtype=torch.float32) for k, v in loss.items()}
                    if isinstance(loss, dict) else torch.tensor(loss, dtype=torch.float32))
            ret = {'decoded': rec['decoded'], 'loss': loss}
            if 'decoded_scores' in rec:
                ret['decoded_scores'] = rec['decoded_scores']
            return ret

    rows = []

    def callback(**kw):
        kw['wer'], kw['cer'] = float(kw['wer']), float(kw['cer'])
        rows.append(kw)

    summary = ref_utils.do_evaluate(Loader(batches), StubModel(), output_callback=callback)
    summary = {k: float(v) for k, v in summary.items()}
    no_callback = ref_utils.do_evaluate(Loader(batches), StubModel())
    assert {k: float(v) for k, v in no_callback.items()} == summary
    print('do_evaluate over the %s: %s' % (how, summary))
    return {'eval_json': np.array(json.dumps(
        {'dataset': how, 'batches': recorded, 'summary': summary, 'rows': rows}))}


def main():
    out = {}
    out.update(make_pairs())
    out.update(make_stats())
    out.update(make_eval())
    path = os.path.join(HERE, 'scoring.npz')
    np.savez_compressed(path, **out)
    print('%s: %d pairs, %d bytes' % (path, len(out['pairs_want']), os.path.getsize(path)))


if __name__ == '__main__':
    main()
