#!/usr/bin/env python
"""tests/golden/make_golden_forced.py — regenerates tests/golden/forced_scores.npz.

Runs ONLY where the reference checkout exists (/root/reference): it imports the reference's own
att_speech.modules.tcn and att_speech.fst_utils under the installed Python (stub modules for the
absent third-party packages, the `beam_search.py[:182]` shim of make_golden_tcn_ff.py) and drives
`AttentionDecoderTCN.enc_initial_state` / `enc_step` and `fst_utils.expand` / `reduce_weights` the
way egs/wsj/local/lattice_search/rescore_lattices2.py and score_groundtruth.py do: per sentence,
batch 1, on the utterance's own frames, the label inputs forced, the alignments summed on top of
the initial one, the log-probabilities of the forced labels and of EOS read one by one and summed
by Python, the LM bag pushed through the sentence and EOS.  Written in this project's words; no
line of the scripts is copied.  Data only.

Two records, `plain_` (no window) and `ff_` (`att_force_forward = (-2, 6)`), at the dimensions
of make_golden_tcn_ff.py (E 16, hidden 24, A 8, 7 symbols, T' = 40, lengths 40 / 23 / 9) with the
toy LM of make_golden.py::_toy_lm (two back-off levels).  Per utterance eight sentences: a
duplicate, a one-label sentence, a proper prefix of another, two that differ only in the last
label.  Stored per record: the state dict, the encoder output, per utterance the sentences (flat
+ lengths) and per sentence `acoustic`, `covered` (frames above coverage_tau), `cov_log` / `cov_count`
(the two scripts' coverage terms), `lm`, `loss_log` / `loss_count`, and the smallest
|coverage - coverage_tau| over every frame of every sentence.  A record is kept only if that margin
is above 1e-3 (the floor of the other generators), so the counts are exact by construction;
otherwise the seed is advanced.

Usage:  python tests/golden/make_golden_forced.py
"""
import importlib.util
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
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
torch.set_num_threads(4)

MARGIN = 1e-3
E, HH, A, S, T, B = 16, 24, 8, 7, 40, 3
LENS = [40, 23, 9]
WINDOW = (-2, 6)
VOCAB = ['<pad>', '<unk>', ' ', 'a', 'b', 'c', 'd']          # 7 symbols; EOS = 7
LM_WEIGHT, COV_TAU, COV_WEIGHT, LEN_NORM = 0.8, 0.1, 0.5, 1.2
KW = dict(tcn_hidden_size=HH, att_hidden_size=A, dropout_p=0.0, kernel_size=3,
          dilation_sizes=[1, 2], beam_size=1, length_normalization=LEN_NORM,
          attention_temperature=1.25, tcn_layers_per_block=2, coverage_tau=COV_TAU,
          coverage_weight=COV_WEIGHT)


def reference_modules():
    from att_speech.configuration import Globals
    Globals.cuda = False
    src = open(os.path.join(REF, 'att_speech/modules/beam_search.py')).read().split('\n')
    ns = {}
    exec(compile('\n'.join(src[:182]), 'beam_search.py[:182]', 'exec'), ns)
    shim = types.ModuleType('att_speech.modules.beam_search')
    shim.BeamSearch = ns['BeamSearch']
    shim.BeamSearchLM = shim.GraphSearch = shim.RescoreSearchLM = object
    sys.modules['att_speech.modules.beam_search'] = shim
    from att_speech import fst_utils as ref_fst
    from att_speech.modules import tcn as ref_tcn
    ref_fst.xrange = range                                   # the file is Python 2
    reduce_py2 = ref_fst.reduce_weights
    ref_fst.reduce_weights = lambda ws, u: reduce_py2(list(ws), u)
    return ref_tcn, ref_fst


def toy_lm():
    """the LM of beam_lm.npz (make_golden.py::_toy_lm) as this build's LmFst, loaded by path"""
    spec = importlib.util.spec_from_file_location(
        'amd_lm_fst', os.path.join(ROOT, 'pytorch-asr_amd/att_speech/lm_fst.py'))
    lm_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lm_mod)
    g = np.load(os.path.join(HERE, 'beam_lm.npz'))
    syms = lm_mod.SymbolTable([(0, '<eps>'), (1, '<spc>'), (2, 'a'), (3, 'b'), (4, 'c')])
    lm = lm_mod.LmFst(6, 0, g['lm_src'], g['lm_dst'], g['lm_il'], g['lm_il'], g['lm_w'],
                      g['lm_final'], syms, syms)
    label_of = {sym: lab for lab, sym in lm.input_symbols()}
    names = ['<spc>' if s == ' ' else s for s in VOCAB + ['<eos>']]
    return lm, [label_of.get(n, label_of['<spc>']) for n in names]


def make_decoder(ref_tcn, seed, window):
    torch.manual_seed(seed)
    dec = ref_tcn.AttentionDecoderTCN({'features': torch.zeros(T, B, E)}, S,
                                      att_force_forward=window,
                                      learnable_initial_attention=window is None, **KW)
    dec.eval()
    with torch.no_grad():
        for prm in dec.parameters():            # make the decoder non-trivial
            prm.add_(torch.randn_like(prm) * 0.1)
        dec.attn.hidden_to_score.weight.normal_(0.0, 0.5)     # peaky, moving alignments
    return dec


def make_sentences(rng):
    """eight per utterance: base, its duplicate, a proper prefix, a last-label variant, one label,
    and three random ones sharing prefixes with the base"""
    out = []
    for _ in range(B):
        base = [int(v) for v in rng.integers(0, S, size=int(rng.integers(4, 7)))]
        variant = base[:-1] + [(base[-1] + 1 + int(rng.integers(0, S - 1))) % S]
        sents = [base, list(base), base[:2], variant, [int(rng.integers(0, S))]]
        for _ in range(3):
            keep = int(rng.integers(0, len(base)))
            tail = [int(v) for v in rng.integers(0, S, size=int(rng.integers(1, 4)))]
            sents.append(base[:keep] + tail)
        order = rng.permutation(len(sents))
        out.append([sents[i] for i in order])
    return out


def forced_pass(dec, ref_fst, lm, mapping, enc_u, len_u, sent):
    """one sentence of one utterance, the two scripts' way"""
    eos = S
    forced = list(sent) + [eos]
    state = dec.enc_initial_state(enc_u, torch.tensor([len_u]), 1, 1)
    summed = state['att_weights'].detach().clone()
    picked = []
    for label in forced:
        fed = state['inputs']
        logits, state = dec.enc_step(**state)
        summed = summed + state['att_weights'].detach()
        picked.append(torch.log_softmax(logits[0][0], dim=-1)[label].item())
        emb = dec.embedding(torch.LongTensor([label])).unsqueeze(0)
        state['inputs'] = torch.cat((fed[1:], emb))
    acoustic = sum(picked)
    above = (summed > dec.coverage_tau).sum(dim=0).float()
    cov_count = (dec.coverage_weight * above).item()
    cov_log = (dec.coverage_weight * torch.log(above / summed.size(0))).item()
    bag = {lm.start(): 0}
    for label in forced:
        bag = ref_fst.expand(lm, bag, mapping[label], use_log_probs=True)
    lm_score = ref_fst.reduce_weights(bag.values(), True) * -LM_WEIGHT
    norm = len(sent) ** dec.length_normalization
    margin = float((summed - dec.coverage_tau).abs().min())
    return dict(acoustic=acoustic, covered=int(above.item()), cov_log=cov_log, cov_count=cov_count,
                lm=lm_score, loss_log=(acoustic + cov_log + lm_score) / norm,
                loss_count=(acoustic + cov_count + lm_score) / norm), margin


def record(ref_tcn, ref_fst, lm, mapping, tag, window, out):
    for seed in range(2020, 2200):
        dec = make_decoder(ref_tcn, seed, window)
        g = torch.Generator().manual_seed(seed + 1000)
        enc = torch.randn(T, B, E, generator=g)
        sentences = make_sentences(np.random.default_rng(seed))
        rec, worst = {}, float('inf')
        with torch.no_grad():
            for u in range(B):
                enc_u = enc[:LENS[u], u:u + 1].contiguous()
                rows = []
                for sent in sentences[u]:
                    vals, margin = forced_pass(dec, ref_fst, lm, mapping, enc_u, LENS[u], sent)
                    worst = min(worst, margin)
                    rows.append(vals)
                rec['u%d_flat' % u] = np.array([c for s in sentences[u] for c in s], np.int64)
                rec['u%d_lens' % u] = np.array([len(s) for s in sentences[u]], np.int64)
                for k in rows[0]:
                    rec['u%d_%s' % (u, k)] = np.array([r[k] for r in rows],
                                                      np.int64 if k == 'covered' else np.float64)
        if worst > MARGIN:
            break
        print('%s seed %d: coverage margin %.2e, reseeding' % (tag, seed, worst))
    else:
        raise SystemExit('no seed with clear coverage margins')
    rec.update(enc=enc.numpy(), seed=np.int32(seed), margin=np.float64(worst))
    for k, v in dec.state_dict().items():
        rec['sd_' + k] = v.detach().numpy().copy()
    out.update({tag + '_' + k: v for k, v in rec.items()})
    print('%s: seed %d, coverage margin %.3g, covered frames %s' % (
        tag, seed, worst, [rec['u%d_covered' % u].tolist() for u in range(B)]))


def main():
    ref_tcn, ref_fst = reference_modules()
    lm, mapping = toy_lm()
    out = {'S': np.int32(S), 'lens': np.array(LENS), 'window': np.array(WINDOW, np.int64),
           'mapping': np.array(mapping), 'lm_weight': np.float64(LM_WEIGHT),
           'coverage_tau': np.float64(COV_TAU), 'coverage_weight': np.float64(COV_WEIGHT),
           'length_normalization': np.float64(LEN_NORM)}
    record(ref_tcn, ref_fst, lm, mapping, 'plain', None, out)
    record(ref_tcn, ref_fst, lm, mapping, 'ff', WINDOW, out)
    path = os.path.join(HERE, 'forced_scores.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
