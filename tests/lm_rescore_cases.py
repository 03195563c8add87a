"""Shared inputs and referees of the LM-rescoring tests (tests/test_lattice_lmrescore.py on the CPU,
tests/test_lattice_lmrescore_gpu.py on the GPU): a random back-off LM generator, an independent scorer of a
word sequence that walks LmFst.arcs() and shares no code with att_speech.lattice_lm.BackoffLm, a complete-path
enumerator for tiny lattices, and the lattices both files rescore."""
import numpy as np
import torch

import nbest_cases as NC
import wfst_cases as WC

from att_speech.lm_fst import LmFst
from att_speech.wfst_decode import DecodingGraph
from att_speech.wfst_lattice import Lattice, decode_lattice

INF = float('inf')
N_WORDS = 8
_CACHE = {}


def random_backoff_lm(rng, n_words=N_WORDS, no_unigram=(3, 7), bigram_share=0.5, trigram_pairs=6, grid=64.0):
    """A back-off LM over the words 1 .. n_words with two back-off levels.  State 0: the unigram state and the
    start; 1: the sink of the sentence-end arcs (no outgoing arcs, final); 2 .. n_words + 1: the bigram
    histories; then `trigram_pairs` trigram histories (w1, w2).  The words in `no_unigram` have no unigram
    (they exist after some histories only).  Final costs are mixed: directly on a state, through a
    sentence-end arc, both, or neither (then the back-off chain decides)."""
    def cost(hi=4.0):
        return float(rng.integers(1, int(hi * grid))) / grid
    U, SINK = 0, 1
    big = {w: 1 + w for w in range(1, n_words + 1)}
    pairs = set()
    while len(pairs) < trigram_pairs:
        pairs.add((int(rng.integers(1, n_words + 1)), int(rng.integers(1, n_words + 1))))
    tri = {p: n_words + 2 + k for k, p in enumerate(sorted(pairs))}
    n = n_words + 2 + len(tri)
    arcs, final = [], np.full(n, INF)
    final[SINK] = cost(1.0)

    def target(hist, w):
        return tri.get((hist, w), big[w]) if hist else big[w]

    def endings(s):
        kind = int(rng.integers(0, 4))
        if kind & 1:
            final[s] = cost()
        if kind & 2:
            arcs.append((s, SINK, 0, cost()))
    for w in range(1, n_words + 1):
        if w not in no_unigram:
            arcs.append((U, big[w], w, cost()))
    arcs.append((U, SINK, 0, cost()))                   # the unigram state always ends a sentence
    for w1 in range(1, n_words + 1):
        s = big[w1]
        arcs.append((s, U, 0, cost(2.0)))               # back-off
        for w2 in range(1, n_words + 1):
            if rng.random() < bigram_share or (w1, w2) in tri:
                arcs.append((s, target(w1, w2), w2, cost()))
        endings(s)
    for (w1, w2), s in tri.items():
        arcs.append((s, big[w2], 0, cost(2.0)))         # back-off to the bigram history
        for w3 in range(1, n_words + 1):
            if rng.random() < 0.4:
                arcs.append((s, target(w2, w3), w3, cost()))
        endings(s)
    src, dst, il, w = zip(*arcs)
    return LmFst(n, U, src, dst, il, il, w, final)


def trivial_lm(n_words=64):
    """one state, every word at cost 0, final cost 0"""
    w = np.arange(1, n_words + 1)
    return LmFst(1, 0, np.zeros(n_words, int), np.zeros(n_words, int), w, w, np.zeros(n_words), np.zeros(1))


def _arcs(lm, s):
    """the arcs of a state, read once from LmFst.arcs() and kept"""
    table = _CACHE.setdefault(('arcs', id(lm)), (lm, {}))[1]      # holds the LM: its id stays its own
    if s not in table:
        table[s] = list(lm.arcs(s))
    return table[s]


def _has_arcs(lm, s):
    return len(_arcs(lm, s)) > 0


def score_words(lm, words):
    """(cost of the words, cost of ending the sentence after them) under the back-off reading, straight from
    LmFst.arcs(); +inf where nothing matches"""
    q, total = lm.start(), 0.0
    for w in words:
        while True:
            arcs = _arcs(lm, q)
            hit = [a for a in arcs if a.ilabel == w]
            if hit:
                total += hit[0].weight
                q = hit[0].nextstate
                break
            bo = [a for a in arcs if a.ilabel == 0 and _has_arcs(lm, a.nextstate)]
            if not bo:
                return INF, INF
            total += bo[0].weight
            q = bo[0].nextstate
    end = 0.0
    while True:
        arcs = _arcs(lm, q)
        stop = min([lm.final(q)] + [a.weight + lm.final(a.nextstate) for a in arcs
                                    if a.ilabel == 0 and not _has_arcs(lm, a.nextstate)])
        if stop < INF:
            return total, end + stop
        bo = [a for a in arcs if a.ilabel == 0 and _has_arcs(lm, a.nextstate)]
        if not bo:
            return total, INF
        end += bo[0].weight
        q = bo[0].nextstate


class TooManyPaths(Exception):
    pass


def complete_paths(lat, limit=20000):
    """every complete path of a lattice as a tuple of lattice arc indices: from the node of time 0 in the
    graph's start state to an end node (time num_frames; a finite final cost when a final state was reached)"""
    if not lat.num_nodes:
        return []
    g = lat.graph
    ptr = np.searchsorted(lat.src, np.arange(lat.num_nodes + 1))
    at_n = lat.time == lat.num_frames
    is_end = at_n & (g.final[lat.state] < INF) if lat.reached_final else at_n
    start = np.nonzero((lat.time == 0) & (lat.state == g.start))[0]
    out = []
    dst = lat.dst.tolist()

    def walk(v, path):
        if is_end[v]:
            out.append(tuple(path))
            if len(out) > limit:
                raise TooManyPaths()
        for j in range(int(ptr[v]), int(ptr[v + 1])):
            path.append(j)
            walk(dst[j], path)
            path.pop()
    for s in start.tolist():
        walk(s, [])
    return out


def path_words(lat, path):
    ol = lat.olabel
    return [int(ol[j]) for j in path if ol[j] != 0]


def path_graph_cost(lat, path):
    """sum of the arc weights plus the final cost of the end state (0 on a partial lattice), in fp64"""
    g = lat.graph
    c = float(np.sum(g.weight[lat.arc[list(path)]].astype(np.float64))) if path else 0.0
    if lat.reached_final:
        v = lat.dst[path[-1]] if path else int(np.nonzero((lat.time == 0) & (lat.state == g.start))[0][0])
        c += float(g.final[lat.state[v]])
    return c


# ---- the lattices -------------------------------------------------------------------------------
BRUTE = [  # (seed, states, T, lens, beam, lattice_beam, final_share)
    (1, 30, 6, [6, 5, 6, 3], 10.0, 6.0, 0.3),
    (4, 40, 5, [5, 5, 4, 1], 10.0, 6.0, 0.3),
    (3, 24, 6, [6, 6, 2, 5], 8.0, 5.0, 0.0),           # no final state: every lattice is partial
]


def brute_case(k):
    """(graph, lattices, LM) of BRUTE[k]"""
    if ('brute', k) not in _CACHE:
        seed, N, T, lens, beam, lb, fs = BRUTE[k]
        rng = np.random.default_rng(seed)
        g = WC.random_graph(rng, N, 3, final_share=fs, n_words=N_WORDS)
        lp = torch.from_numpy(WC.grid_scores(rng, T, len(lens), 3, lens, low=-4.0))
        lats = decode_lattice(lp, lens, g, beam=beam, lattice_beam=lb)[0]
        _CACHE[('brute', k)] = (g, lats, random_backoff_lm(rng))
    return _CACHE[('brute', k)]


SHIPPED_LENS = [12, 12, 9]


def shipped_case():
    """(graph HC o bigram, lattices, trigram LmFst, label map): 12 frames, 3 utterances, beam 8, lattice beam 4"""
    if 'shipped' not in _CACHE:
        from att_speech.lattice_lm import lm_label_map
        g = NC.bigram_graph()
        tg = LmFst.read(NC.BIGRAM_LM.replace('_bg_', '_tg_'))
        torch.manual_seed(0)
        lp = torch.log_softmax(torch.randn(12, 3, 49), -1)
        lats = decode_lattice(lp, SHIPPED_LENS, g, beam=8.0, lattice_beam=4.0)[0]
        _CACHE['shipped'] = (g, lats, tg, lm_label_map(tg, NC.WSJ_VOCAB, 49))
    return _CACHE['shipped']


def bigram_lm():
    return LmFst.read(NC.BIGRAM_LM)


def fan(n, n_words=N_WORDS, seed=0):
    """A lattice of n nodes in three levels: the start node, n - 2 middle nodes and one end node that has
    n - 2 in-arcs; the first arcs carry words, so the end node collects many LM states."""
    rng = np.random.default_rng(seed)
    m = n - 2
    src = np.r_[np.zeros(m, int), np.arange(1, m + 1)]
    dst = np.r_[np.arange(1, m + 1), np.full(m, n - 1)]
    ol = np.r_[rng.integers(1, n_words + 1, m), rng.integers(0, n_words + 1, m)]
    il = np.r_[np.ones(m, int), np.full(m, 2)]
    w = rng.integers(0, 256, 2 * m) / 64.0
    final = np.full(n, INF)
    final[n - 1] = 0.5
    g = DecodingGraph(n, 0, src, dst, il, ol, w, final)
    assert (g.src == src).all()
    lp = -(rng.integers(0, 64, 2 * m) / 16.0).astype(np.float32)
    time = np.r_[0, np.ones(m, int), 2]
    zeros = np.zeros(n, np.float32)
    return Lattice(g, 1.0, 2, 0.0, True, time, np.arange(n), zeros, zeros, g.src, g.dst, np.arange(2 * m), lp)


def fan_lm():
    """every word after every word: the end node of fan(n) holds one LM state per last word"""
    if 'fan_lm' not in _CACHE:
        _CACHE['fan_lm'] = random_backoff_lm(np.random.default_rng(11), no_unigram=(), bigram_share=1.0)
    return _CACHE['fan_lm']
