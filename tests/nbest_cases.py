"""Shared inputs and checks of the n-best tests (tests/test_lattice_nbest.py on the CPU,
tests/test_lattice_nbest_gpu.py on the GPU): the toy sweep of tests/wfst_cases.py, unquantised scores
over the shipped bigram LM graph, and a hand-made lattice with thousands of arcs at one node."""
import numpy as np
import torch

from grammar_cases import BIGRAM_LM, WSJ_VOCAB
from wfst_cases import INF, TOYS, grid_scores, toy_graph

from att_speech.wfst_decode import DecodingGraph
from att_speech.wfst_lattice import Lattice, decode_lattice

LENS = [5, 1, 3, 5]
SCALES = (1.0, 0.5)
LATTICE_BEAMS = (0.0, 1.0, 2.0, 4.0, INF)
SMALL_N = (1, 2, 3, 10)

_CACHE = {}


def toy_inputs(name):
    return toy_graph(name), grid_scores(np.random.default_rng(len(name) + 3), 5, 4, 3, LENS, low=-4.0)


def toy_lattices(name, scale, lb):
    """the four host lattices of a toy, and per lattice Lattice.nbest(10**6): every sequence"""
    key = ('toy', name, scale, lb)
    if key not in _CACHE:
        g, lp = toy_inputs(name)
        lats = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF, lattice_beam=lb, acoustic_scale=scale)[0]
        _CACHE[key] = (lats, [lat.nbest(10 ** 6) for lat in lats])
    return _CACHE[key]


def sweep():
    """(name, scale, lattice_beam) of the toy sweep"""
    return [(name, scale, lb) for name in sorted(TOYS) for scale in SCALES for lb in LATTICE_BEAMS]


def sweep_ns(every):
    """the list lengths of the sweep for lattices whose complete lists are `every`"""
    return SMALL_N + (max(len(e) for e in every) + 5,)


def bigram_graph():
    if 'bigram' not in _CACHE:
        from att_speech import fst_utils
        gg = fst_utils.CTCGraphGen(context_order=1, num_symbols=49, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
        _CACHE['bigram'] = DecodingGraph.from_graph_generator(gg)
    return _CACHE['bigram']


UNQUANTISED_LENS = [24, 17, 9, 1]
UNQUANTISED_BEAMS = (2.0, 4.0, 6.0)


def unquantised_scores():
    torch.manual_seed(1)
    return torch.log_softmax(3 * torch.randn(24, 4, 49), -1)


def unquantised_lattices(lb):
    key = ('unq', lb)
    if key not in _CACHE:
        _CACHE[key] = decode_lattice(unquantised_scores(), UNQUANTISED_LENS, bigram_graph(), beam=16.0,
                                     lattice_beam=lb)[0]
    return _CACHE[key]


def fan_lattice(F=3000):
    """One lattice made by hand, three frames: a hub with 2 F arcs out to F middle nodes (two
    parallel arcs each), F arcs from those into one sink, three parallel arcs from the sink to the
    end.  Weights and scores sit on a coarse grid, so costs tie in hundreds; output labels repeat
    (and some are 0), so most candidates at the hub are duplicates of a sequence already listed.
    States are numbered by depth, so node = state and the lattice arcs are the graph's."""
    if ('fan', F) in _CACHE:
        return _CACHE['fan', F]
    rng = np.random.default_rng(11)
    hub, sink, end = 0, F + 1, F + 2
    mid = np.arange(1, F + 1)
    src = np.concatenate([np.repeat(hub, 2 * F), mid, [sink] * 3])
    dst = np.concatenate([mid, mid, np.repeat(sink, F), [end] * 3])
    il = np.concatenate([rng.integers(1, 4, 2 * F), rng.integers(1, 4, F), [1, 2, 3]])
    ol = np.concatenate([rng.integers(0, 40, 2 * F), rng.integers(0, 30, F) + 100 * (rng.random(F) < 0.8), [7, 0, 8]])
    ol = np.where(ol == 100, 0, ol)
    w = np.concatenate([rng.integers(0, 4, 2 * F) / 4.0, rng.integers(0, 3, F) / 4.0, [0.25, 0.25, 0.5]])
    final = np.full(F + 3, INF)
    final[end] = 0.5
    perm = rng.permutation(len(src))
    g = DecodingGraph(F + 3, 0, src[perm], dst[perm], il[perm], ol[perm], w[perm], final)
    depth = np.zeros(F + 3, np.int32)
    depth[mid], depth[sink], depth[end] = 1, 2, 3
    G = len(g.src)
    assert (np.diff(g.src) >= 0).all()                  # CSR: lattice arcs by (source node, graph arc)
    lp = -(rng.integers(0, 3, G) / 2.0).astype(np.float32)
    zeros = np.zeros(F + 3, np.float32)
    lat = Lattice(g, 1.0, 3, 0.0, True, depth, np.arange(F + 3), zeros, zeros, g.src, g.dst, np.arange(G), lp)
    _CACHE['fan', F] = lat
    return lat


def without_words(lat):
    """the same lattice over a copy of its graph whose output labels are all 0"""
    import copy
    g = copy.copy(lat.graph)
    g.olabel = np.zeros_like(lat.graph.olabel)
    g._device = {}
    return Lattice(g, lat.acoustic_scale, lat.num_frames, lat.cost, lat.reached_final,
                   *[getattr(lat, f) for f in Lattice.FIELDS])


def check_against_host(got, lat, every, n, what):
    """one utterance's list against Lattice.nbest: what tests/test_lattice_nbest.py promises"""
    want = lat.nbest(n)
    assert [c for _, c in got] == [c for _, c in want], (what, got, want)
    seqs = [tuple(w) for w, _ in got]
    assert len(set(seqs)) == len(seqs), what
    cost_of = {tuple(w): c for w, c in every}
    assert all(cost_of[s] == c for s, (_, c) in zip(seqs, got)), what
    if got:
        assert {tuple(w) for w, c in every if c < got[-1][1]} <= set(seqs), what
    assert got == sorted(got, key=lambda e: (e[1], e[0])), what
    if n >= len(every):
        assert got == want == every, what
