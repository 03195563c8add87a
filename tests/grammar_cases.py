"""Shared pieces of the grammar-graph tests (tests/test_grammar_graphs.py on the CPU,
tests/test_lattice_shared_gpu.py on the GPU): toy back-off LMs, an independent fp64 scorer of
G, and a torch evaluation of the reference's path_reduction on padded matrices."""
import os

import numpy as np
import torch

from conftest import GOLDEN

BIGRAM_LM = os.path.join(GOLDEN, 'G_char_bg_syms.fst.gz')
TRIGRAM_LM = os.path.join(GOLDEN, 'G_char_tg_syms.fst.gz')
WSJ_VOCAB = os.path.join(GOLDEN, 'wsj_vocabulary.txt')
INF = float('inf')


def toy_lm(kind):
    """Back-off LMs over the tropical weight set with the reference's table layout
    (<eps>, <s>, </s>, then the symbols).  Returns (LmFst, network vocabulary).

    's3': symbols a, b.  State 3 is the unigram back-off state, 4 has no way in, 5 no way out
    (so `b` is accepted only as the first symbol); `a` after `a` has a direct arc AND a
    back-off path to the same state (they add up).
    's4': symbols ' ', a, b with a two-level back-off chain 1,2 -> 3 -> 4 and a state (5)
    that nothing reaches; ' ' is accepted only after `b`."""
    from att_speech.lm_fst import LmFst, SymbolTable
    if kind == 's3':
        vocab = ['<pad>', 'a', 'b']
        syms = SymbolTable([(0, '<eps>'), (1, '<s>'), (2, '</s>'), (3, 'b'), (4, 'a')])
        a, b = 4, 3
        arcs = [(0, 1, a, 0.7), (0, 2, b, 1.2), (0, 3, 0, 0.3), (1, 1, a, 0.9), (1, 3, 0, 0.5),
                (2, 1, a, 0.4), (2, 3, 0, 0.8), (3, 1, a, 1.5), (1, 5, b, 2.0),
                (4, 3, a, 0.1)]
        final = [2.0, 0.6, INF, 1.0, 0.2, INF]
    else:
        vocab = ['<pad>', ' ', 'a', 'b']
        syms = SymbolTable([(0, '<eps>'), (1, '<s>'), (2, '</s>'), (3, 'a'), (4, '<spc>'), (5, 'b')])
        sp, a, b = 4, 3, 5
        arcs = [(0, 1, a, 0.9), (0, 4, 0, 0.2), (1, 2, b, 0.5), (1, 1, a, 1.4), (1, 3, 0, 0.7),
                (2, 0, sp, 0.3), (2, 3, 0, 0.6), (3, 2, b, 1.0), (3, 4, 0, 0.4), (4, 1, a, 1.3),
                (4, 2, b, 1.6), (5, 1, a, 0.1), (2, 2, b, 2.2)]
        final = [0.5, INF, 1.1, INF, 2.5, 0.0]
    src, dst, il, w = [np.array(x) for x in zip(*arcs)]
    return LmFst(len(final), 0, src, dst, il, il, w, np.array(final, np.float64), syms, syms), vocab


def lm_matrices(lm, glabel):
    """(closure K = (I - E)^-1 of the epsilon arcs, {network symbol: arc matrix}, final vector),
    all in the probability domain, fp64: an evaluation of G that shares nothing with the builder
    (no ranks, no level order)."""
    n = lm.num_states()
    eps = np.zeros((n, n))
    by = {}
    for s, d, l, w in zip(lm.src, lm.dst, lm.ilabel, lm.weight):
        if l == 0:
            eps[s, d] += np.exp(-w)
        elif glabel[l] > 0:
            by.setdefault(int(glabel[l]), np.zeros((n, n)))[s, d] += np.exp(-w)
    return np.linalg.inv(np.eye(n) - eps), by, np.exp(-lm.final_w)


def lm_log_score(lm, glabel, y, mats=None):
    """log G(y), -inf when G does not accept y"""
    K, by, fin = mats or lm_matrices(lm, glabel)
    n = lm.num_states()
    v = np.zeros(n); v[lm.start()] = 1.0
    v = v @ K
    for l in y:
        if int(l) not in by:
            return -INF
        v = v @ by[int(l)] @ K
    tot = float(v @ fin)
    return np.log(tot) if tot > 0 else -INF


def torch_path_reduction(log_probs, act_lens, graph_matrices, red_kind='logsumexp', neg_inf=-1e20):
    """The reference's path_reduction (att_speech/fst_utils.py:349-397) on the 4 in-edge
    matrices, differentiable, in the dtype of `log_probs` (CPU)."""
    states, ilabels, weights, term = [m.expand(log_probs.size(1), -1, -1) for m in graph_matrices[:4]]
    weights, term = weights.to(log_probs.dtype), term.to(log_probs.dtype)
    bs, n, k = states.shape

    def red(t):
        return torch.logsumexp(t, -1) if red_kind == 'logsumexp' else t.max(-1)[0]
    alpha = torch.full((bs, n), neg_inf, dtype=log_probs.dtype)
    alpha[:, 0] = 0
    lens = torch.as_tensor(act_lens)
    for t in range(log_probs.size(0)):
        tok = (torch.gather(alpha, 1, states.reshape(bs, -1)).view(bs, n, k) + weights +
               torch.gather(log_probs[t], 1, ilabels.reshape(bs, -1)).view(bs, n, k))
        alpha = torch.where((t < lens)[:, None], red(tok), alpha)
    return red(alpha + term.squeeze(2))
