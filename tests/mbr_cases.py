"""Shared inputs of the minimum-Bayes-risk tests (tests/test_lattice_mbr.py on the CPU,
tests/test_lattice_mbr_gpu.py on the GPU): the lattices of tests/nbest_cases.py, a hand-made tree, a
single path, and an utterance long enough for a hypothesis of more than 32 words."""
import numpy as np
import torch

import nbest_cases as NC
from wfst_cases import INF

from att_speech.wfst_decode import DecodingGraph
from att_speech.wfst_lattice import Lattice, decode_lattice

_CACHE = {}


def tree_lattice():
    """Depth 4, branching 2, 3, 2, 3 (57 nodes, 36 leaves = 36 paths); every node has one in-arc, so
    the recursion's expected distances are exact.  Words on some arcs, 0 on others, words repeat.
    States are numbered by depth, so node = state and the lattice arcs are the graph's."""
    if 'tree' in _CACHE:
        return _CACHE['tree']
    rng = np.random.default_rng(5)
    depth, src, dst = [0], [], []
    level = [0]
    for d, fan in enumerate((2, 3, 2, 3), 1):
        nxt = []
        for u in level:
            for _ in range(fan):
                v = len(depth)
                depth.append(d)
                src.append(u), dst.append(v), nxt.append(v)
        level = nxt
    n, A = len(depth), len(src)
    ol = rng.integers(0, 5, A)                  # 0: no word; 1 .. 4 repeat all over the tree
    il = rng.integers(1, 4, A)
    w = rng.integers(0, 8, A) / 4.0
    final = np.full(n, INF)
    final[level] = rng.integers(0, 4, len(level)) / 4.0
    g = DecodingGraph(n, 0, src, dst, il, ol, w, final)
    assert (g.src == np.asarray(src)).all()
    lp = -(rng.integers(0, 6, A) / 4.0).astype(np.float32)
    zeros = np.zeros(n, np.float32)
    lat = Lattice(g, 1.0, 4, 0.0, True, np.asarray(depth, np.int32), np.arange(n), zeros, zeros, g.src, g.dst,
                  np.arange(A), lp)
    _CACHE['tree'] = lat
    return lat


def single_path():
    """five arcs in a row, words 3, 0, 4, 4, 2"""
    if 'single' not in _CACHE:
        ol = [3, 0, 4, 4, 2]
        final = np.full(6, INF)
        final[5] = 0.25
        g = DecodingGraph(6, 0, np.arange(5), np.arange(1, 6), [1, 2, 1, 3, 2], ol, [0.5, 0.25, 1.0, 0.0, 0.75], final)
        zeros = np.zeros(6, np.float32)
        lp = np.asarray([-0.5, -1.0, -0.25, -2.0, -0.75], np.float32)
        _CACHE['single'] = Lattice(g, 1.0, 5, 0.0, True, np.arange(6), np.arange(6), zeros, zeros, g.src, g.dst,
                                   np.arange(5), lp)
    return _CACHE['single']


LONG_LENS = [150, 1]


def long_inputs():
    """150 frames over the bigram LM graph: the best path holds more than 32 words"""
    torch.manual_seed(3)
    return NC.bigram_graph(), torch.log_softmax(3 * torch.randn(150, 2, 49), -1)


def long_lattices():
    if 'long' not in _CACHE:
        g, lp = long_inputs()
        _CACHE['long'] = decode_lattice(lp, LONG_LENS, g, beam=16.0, lattice_beam=2.0)[0]
    return _CACHE['long']


def toy_sweep():
    """(name, scale, lattice_beam) of nbest_cases' toy sweep, all of it"""
    return NC.sweep()


def toy_cases():
    return [('toy %s %s %s #%d' % (name, scale, lb, b), lat) for name, scale, lb in toy_sweep()
            for b, lat in enumerate(NC.toy_lattices(name, scale, lb)[0])]


def enumerable():
    """[(name, lattice)] small enough for the path enumerator: the hand-made ones and the whole toy sweep"""
    return [('tree', tree_lattice()), ('single', single_path()),
            ('silent', NC.without_words(tree_lattice()))] + toy_cases()


def all_lattices():
    """[(name, lattice)]: every case lattice"""
    out = enumerable() + [('fan', NC.fan_lattice()), ('long', long_lattices()[0])]
    for b, lat in enumerate(NC.unquantised_lattices(4.0)):
        out.append(('unquantised #%d' % b, lat))
    return out


def probe_hypotheses(lat):
    """the sentences a lattice is scored against: its five best, the empty one, one with a foreign word"""
    hyps = [list(w) for w, _ in lat.nbest(5)] if lat.num_nodes else []
    foreign = int(lat.graph.olabel.max()) + 7
    return hyps + [[], (hyps[0][:1] if hyps else []) + [foreign] + (hyps[0][1:] if hyps else [])]
