"""Dev-set evaluation measurement (development tool; bench.py is the contract benchmark): the
DeepSpeech2 encoder + greedy CTCDecoderAdvanced on the mono model (49 symbols) at B = 64 on
bench.synthetic_batch-style inputs with 100-character reference texts.  Reports utterances/s of
`model.decode` alone (the yardstick: code that does not change with the scorer), of
`utils.do_evaluate` with the native scorer (asr_edit_distance_stats_i32, one launch per batch)
and of `utils.do_evaluate` with ASR_NATIVE_SCORING=0 (the host implementation), alternating in
one process, medians over the rounds; and where do_evaluate's host time goes (tokenisation,
packing).  Measured twice: with the untrained model's own greedy output (nearly empty
hypotheses, the scorer's easy case) and with `model.decode` still running but reporting
perturbed copies of the references (about 10 % edits), so that every character pair is
100 x 100 as after training.  --only native runs the native path alone on the perturbed
hypotheses, for a kernel trace
(`rocprofv3 --kernel-trace --stats -- python tools/bench_scoring.py --only native`).
--json writes the result as one JSON document."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('MIOPEN_USER_DB_PATH', os.path.join(ROOT, 'pytorch-asr_amd', 'miopen_db'))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-asr_amd'))
sys.path.insert(0, ROOT)

import bench                                   # noqa: E402  (model_config)
from att_speech import utils                    # noqa: E402
from att_speech.models import SpeechModel       # noqa: E402

S = 49
SWITCH = 'ASR_NATIVE_SCORING'
CTC_DEC = dict(class_name='att_speech.modules.decoders.advanced_decoder.CTCDecoderAdvanced')


class Dataset(object):
    """ids -> characters -> words the way the WSJ recipes' dataset does it: one symbol per id, id 2
    the space, id 29 the noise symbol that `ignore_noise` drops"""
    itos = ['<pad>', '<unk>', ' '] + [chr(ord('A') + i % 26) for i in range(S - 3)]
    NOISE = 29

    def ids_to_chars_words_sentence(self, text_ids, ignore_noise=False):
        symbols = [self.itos[i] for i in text_ids if not (ignore_noise and i == self.NOISE)]
        text = ''.join(symbols)
        return symbols, text.split(), text


class Loader(list):
    dataset = Dataset()


def make_loader(nbatches, B, T, L):
    g = torch.Generator().manual_seed(1234)
    out = []
    for j in range(nbatches):
        texts = torch.randint(3, S, (B, L), generator=g, dtype=torch.int32)
        texts[:, 5::6] = 2                      # a word every six characters: 17 words
        out.append({'uttids': ['u%d_%d' % (j, b) for b in range(B)], 'spkids': None,
                    'features': (torch.randn(B, T, 40, 1, generator=g),
                                 torch.full((B,), T, dtype=torch.int32)),
                    'texts': (texts, torch.full((B,), L, dtype=torch.int32)), 'ivectors': None})
    return Loader(out)


def perturbed_references(loader, rate=0.1):
    """per batch (keyed by the address of its text tensor): every reference text with about
    `rate` of its positions substituted, dropped or doubled — hypotheses of a trained model's
    length, so that the scorer works at its nominal 100 x 100 size"""
    rnd = random.Random(99)
    out = {}
    for batch in loader:
        hyps = []
        for row in batch['texts'][0].tolist():
            h = []
            for tok in row:
                r = rnd.random()
                if r < rate / 3:
                    continue
                h.append(rnd.randrange(2, S) if r < 2 * rate / 3 else tok)
                if r > 1 - rate / 3:
                    h.append(tok)
            hyps.append(h)
        out[batch['texts'][0].data_ptr()] = hyps
    return out


def substitute_hypotheses(model, table):
    """`model.decode` still runs (its cost is the yardstick) but reports `table`'s label lists"""
    real = model.decode

    def decode(features, feature_lens, speakers, texts, *a, **kw):
        ret = real(features, feature_lens, speakers, texts, *a, **kw)
        ret['decoded'] = table[texts.data_ptr()]
        return ret
    model.decode = decode


def decode_only(loader, model, dev):
    for batch in loader:
        model.decode(batch['features'][0].to(dev), batch['features'][1], batch['spkids'],
                     batch['texts'][0], batch['texts'][1], ivectors=None)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    fn()
    torch.cuda.synchronize()
    return time.time() - t0


def host_breakdown(loader, model, dev):
    """milliseconds per batch of do_evaluate's own host steps, on the first batch's decode output"""
    batch = loader[0]
    out = model.decode(batch['features'][0].to(dev), batch['features'][1], None,
                       batch['texts'][0], batch['texts'][1])['decoded']
    tokeniser = loader.dataset.ids_to_chars_words_sentence
    torch.cuda.synchronize()
    t0 = time.time()
    hyp = [tokeniser(e, ignore_noise=True) for e in out]
    rows, ns = batch['texts'][0].tolist(), batch['texts'][1].tolist()
    ref = [tokeniser(rows[i][:ns[i]], ignore_noise=True) for i in range(len(out))]
    t1 = time.time()
    hyps = [h[1] for h in hyp] + [h[0] for h in hyp]
    refs = [r[1] for r in ref] + [r[0] for r in ref]
    os.environ[SWITCH] = '1'
    counts = utils._score_pairs(hyps, refs, dev)
    t2 = time.time()
    torch.cuda.synchronize()
    assert isinstance(counts, torch.Tensor)
    os.environ[SWITCH] = '0'
    t3 = time.time()
    utils._score_pairs(hyps, refs, dev)
    t4 = time.time()
    os.environ.pop(SWITCH, None)
    return {'tokenise_ms': round((t1 - t0) * 1e3, 3),
            'native_pack_and_launch_ms': round((t2 - t1) * 1e3, 3),
            'host_scoring_ms': round((t4 - t3) * 1e3, 3),
            'mean_hypothesis_chars': round(sum(len(h[0]) for h in hyp) / len(hyp), 1)}


def measure(loader, model, dev, rounds):
    n = sum(len(b['uttids']) for b in loader)

    def evaluate(native):
        os.environ[SWITCH] = '1' if native else '0'
        return utils.do_evaluate(loader, model)

    s_native, s_host = evaluate(True), evaluate(False)
    assert all(float(s_native[k]) == float(s_host[k]) for k in s_native), (s_native, s_host)
    rates = {'decode': [], 'evaluate_native': [], 'evaluate_host': []}
    for _ in range(rounds):
        rates['decode'].append(n / timed(lambda: decode_only(loader, model, dev)))
        rates['evaluate_native'].append(n / timed(lambda: evaluate(True)))
        rates['evaluate_host'].append(n / timed(lambda: evaluate(False)))
    os.environ.pop(SWITCH, None)
    med = {k: statistics.median(v) for k, v in rates.items()}
    return {'utt_per_s': {k: round(v, 1) for k, v in med.items()},
            'utt_per_s_rounds': {k: [round(x, 1) for x in v] for k, v in rates.items()},
            'evaluate_native_extra_wall_time': round(med['decode'] / med['evaluate_native'] - 1.0, 4),
            'evaluate_host_extra_wall_time': round(med['decode'] / med['evaluate_host'] - 1.0, 4),
            'host_steps_per_batch': host_breakdown(loader, model, dev),
            'CER': float(s_native['CER']), 'WER': float(s_native['WER'])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--chars', type=int, default=100)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', choices=['native'], default=None,
                    help='native path alone, perturbed-reference hypotheses (kernel trace)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B, T = a.batch, a.frames
    enc_cfg, _ = bench.model_config(1, None)
    loader = make_loader(a.batches, B, T, a.chars)
    sample = {'features': loader[0]['features'][0][:2].clone(),
              'features_lengths': loader[0]['features'][1][:2].clone(), 'spkids': None}
    torch.manual_seed(0)
    model = SpeechModel(enc_cfg, dict(CTC_DEC), sample, S, [str(i) for i in range(S)]).to(dev).eval()
    decode_only(loader, model, dev)             # warm up
    result = {'B': B, 'frames': T, 'chars': a.chars, 'batches': a.batches, 'rounds': a.rounds}
    if not a.only:
        # the untrained model's own greedy output: nearly empty hypotheses, the scorer's easy case
        result['greedy_hypotheses'] = measure(loader, model, dev, a.rounds)
    substitute_hypotheses(model, perturbed_references(loader))
    if a.only:
        os.environ[SWITCH] = '1'
        summary = utils.do_evaluate(loader, model)
        print(json.dumps({'only': a.only, 'CER': float(summary['CER'])}))
        return
    result['perturbed_reference_hypotheses'] = measure(loader, model, dev, a.rounds)
    print(json.dumps(result))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
