"""Shared pieces of tests/test_forced_scores.py and tests/test_forced_scores_gpu.py: the golden
record of tests/golden/forced_scores.npz (made by tests/golden/make_golden_forced.py from the
reference's own decoder and LM functions) as a model of this build plus its sentences and expected
scores, and a brute-force restatement of the prefix trie."""
import os

import numpy as np
import torch

import lm_beam_referee as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'forced_scores.npz')
VOCAB = ['<pad>', '<unk>', ' ', 'a', 'b', 'c', 'd']
KEYS = ('acoustic', 'covered', 'cov_log', 'cov_count', 'lm', 'loss_log', 'loss_count')
_CACHE = {}


def golden():
    if 'g' not in _CACHE:
        _CACHE['g'] = dict(np.load(GOLDEN))
    return _CACHE['g']


def golden_decoder(tag):
    """the decoder of record `tag` ('plain' / 'ff'), on the CPU in eval mode"""
    from att_speech.modules.tcn import AttentionDecoderTCN
    g = golden()
    window = tuple(int(v) for v in g['window']) if tag == 'ff' else None
    dec = AttentionDecoderTCN(
        {'features': torch.zeros(40, 3, 16)}, int(g['S']), tcn_hidden_size=24, att_hidden_size=8,
        dropout_p=0.0, kernel_size=3, dilation_sizes=[1, 2], beam_size=1, tcn_layers_per_block=2,
        attention_temperature=1.25, att_force_forward=window,
        learnable_initial_attention=window is None, vocabulary=VOCAB, lm_file=lr.toy_lm(),
        lm_weight=float(g['lm_weight']), coverage_tau=float(g['coverage_tau']),
        coverage_weight=float(g['coverage_weight']),
        length_normalization=float(g['length_normalization']))
    assert list(dec.alphabet_mapping) == g['mapping'].tolist()
    sd = {k[len(tag) + 4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(tag + '_sd_')}
    dec.load_state_dict(sd)
    return dec.eval()


def golden_inputs(tag):
    """-> (encoded [40, 3, 16], lens, sentences per utterance, expected {key: [per utterance]})"""
    g = golden()
    sentences, want = [], {k: [] for k in KEYS}
    for u in range(3):
        flat, lens = g['%s_u%d_flat' % (tag, u)], g['%s_u%d_lens' % (tag, u)]
        cuts = np.cumsum(lens)[:-1]
        sentences.append([[int(c) for c in s] for s in np.split(flat, cuts)])
        for k in KEYS:
            want[k].append(g['%s_u%d_%s' % (tag, u, k)])
    return torch.from_numpy(g[tag + '_enc']), torch.from_numpy(g['lens']), sentences, want


def brute_trie(sentences, eos):
    """level -> sorted distinct prefixes of that length that some sentence + [EOS] extends"""
    full = sorted({tuple(s) + (eos,) for s in sentences})
    depth = max(len(f) for f in full)
    return full, [sorted({f[:l] for f in full if len(f) > l}) for l in range(depth)]


def unit_prefixes(trie):
    """the prefix of every unit of every level, rebuilt by walking the parents"""
    out = []
    for l, lv in enumerate(trie['levels']):
        if l == 0:
            out.append([()])
            continue
        out.append([out[l - 1][int(p)] + (int(c),) for p, c in zip(lv['parent'], lv['label'])])
    return out


def check_trie(sentences, eos):
    """every property of the trie of one utterance; returns it"""
    from att_speech.modules.beam_search import sentence_trie
    trie = sentence_trie(sentences, eos)
    full, want_levels = brute_trie(sentences, eos)
    prefixes = unit_prefixes(trie)
    assert trie['count'] == len(full) and len(trie['levels']) == len(want_levels)
    finished = {}
    for l, lv in enumerate(trie['levels']):
        # the units of a level are exactly its distinct prefixes
        assert lv['n_units'] == len(prefixes[l]) == len(set(prefixes[l]))
        assert sorted(prefixes[l]) == want_levels[l]
        ptr = lv['edge_ptr']
        assert len(ptr) == lv['n_units'] + 1 and ptr[0] == 0 and ptr[-1] == len(lv['edge_dst'])
        assert (np.diff(ptr) >= 1).all()                     # a unit without an edge cannot exist
        made = []
        for unit in range(lv['n_units']):
            for e in range(ptr[unit], ptr[unit + 1]):
                lab, dst = int(lv['edge_label'][e]), int(lv['edge_dst'][e])
                if dst >= 0:
                    assert lab != eos and prefixes[l + 1][dst] == prefixes[l][unit] + (lab,)
                    made.append(dst)
                else:
                    assert lab == eos and -1 - dst not in finished
                    finished[-1 - dst] = prefixes[l][unit]   # the walk up from the EOS edge
        if l + 1 < len(trie['levels']):
            assert sorted(made) == list(range(trie['levels'][l + 1]['n_units']))
        else:
            assert not made
    # every distinct sentence has one EOS edge, which rebuilds it; duplicates share it
    assert sorted(finished) == list(range(len(full)))
    for given, s in zip(sentences, trie['inverse']):
        assert finished[int(s)] == tuple(given)
        assert trie['lengths'][int(s)] == len(given)
    return trie


# ------------------------------------------------------------------ the launch, restated

def forced_level_ref(logits, att, cov_in, parent, edge_ptr, edge_label, edge_dst, acoustic_in, lens,
                     B, width, tau, n_out, n_sent, dtype=np.float64):
    """asr_forced_level_f32 from the header, in numpy: -> dict(cov_out fp32 (one fp32 add),
    acoustic_out [n_out], sent_acoustic / sent_covered [n_sent], written masks, and `terms`, the
    log-probability of every edge in `dtype` (fp64: the exact value of the fp32 logits))."""
    logits, att, cov_in = np.asarray(logits), np.asarray(att, np.float32), np.asarray(cov_in, np.float32)
    slots, C = logits.shape
    T = att.shape[1]
    assert slots == B * width
    cov_out = (cov_in[np.asarray(parent)] + att).astype(np.float32)
    x = logits.astype(dtype)
    m = x.max(1, keepdims=True)
    logp = (x - m) - np.log(np.exp(x - m).sum(1, keepdims=True))
    out = dict(cov_out=cov_out, acoustic_out=np.zeros(n_out), sent_acoustic=np.zeros(n_sent),
               sent_covered=np.zeros(n_sent, np.int64), out_written=np.zeros(n_out, bool),
               sent_written=np.zeros(n_sent, bool), terms=np.zeros(len(edge_dst)),
               cov_margin=np.inf)
    for p in range(slots):
        ln = int(lens[p // width])
        if edge_ptr[p] < edge_ptr[p + 1]:
            out['cov_margin'] = min(out['cov_margin'],
                                    float(np.abs(cov_out[p, :ln].astype(np.float64) - tau).min()))
        for e in range(edge_ptr[p], edge_ptr[p + 1]):
            term = float(logp[p, edge_label[e]])
            out['terms'][e] = term
            v = float(acoustic_in[p]) + term
            d = int(edge_dst[e])
            if d >= 0:
                assert not out['out_written'][d]
                out['acoustic_out'][d], out['out_written'][d] = v, True
            else:
                s = -1 - d
                assert not out['sent_written'][s]
                out['sent_acoustic'][s], out['sent_written'][s] = v, True
                out['sent_covered'][s] = int((cov_out[p, :ln] > np.float32(tau)).sum())
    return out
