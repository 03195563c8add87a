"""att_speech.wfst_lattice on the CPU: the numpy host path of decode_lattice against the dense fp64
referee (tests/wfst_lattice_referee.py) in every canonical field, the lattice against brute-force
path enumeration, and best_path / nbest / FSTDecoder / tools/decode_graph.py on top of it.

Inputs sit on the 2^-8 grid of tests/wfst_cases.py: every fp32 sum is exact, so fp32 must equal
fp64 in every bit.  Frames beyond an utterance's length are NaN."""
import os
import sys

import numpy as np
import pytest
import torch

import wfst_lattice_referee as LR
import wfst_referee as R
from grammar_cases import BIGRAM_LM, WSJ_VOCAB
from wfst_cases import INF, TOYS, grid_scores, toy_graph

from att_speech.wfst_decode import decode_graph
from att_speech.wfst_lattice import Lattice, best_paths, decode_lattice

LENS = [5, 1, 3, 5]
LATTICE_BEAMS = (0.0, 1.0, 2.0, 4.0, INF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def toy_case(name):
    g = toy_graph(name)
    lp = grid_scores(np.random.default_rng(len(name) + 3), 5, 4, 3, LENS, low=-4.0)
    return g, lp


@pytest.mark.parametrize('name', sorted(TOYS))
def test_host_path_equals_the_referee(name):
    g, lp = toy_case(name)
    for scale in (1.0, 0.5):
        for beam in (INF, 1.0):
            for lb in LATTICE_BEAMS:
                kw = dict(beam=beam, lattice_beam=lb, acoustic_scale=scale)
                lats, redone = decode_lattice(torch.from_numpy(lp), LENS, g, **kw)
                assert redone == [] and all(isinstance(l, Lattice) for l in lats)
                want = LR.lattices(R.graph_args(g), lp, LENS, **kw)
                for b in range(len(LENS)):
                    LR.assert_same(lats[b], want[b], (name, kw, b))
                    assert lats[b].alpha.dtype == np.float32 and lats[b].lp.dtype == np.float32


def _lattice_paths(lat):
    """every complete path of a lattice as a tuple of graph arc indices (toy lattices only)"""
    out_arcs = [[] for _ in range(lat.num_nodes)]
    for j in range(lat.num_arcs):
        out_arcs[lat.src[j]].append(j)
    ends = (lat.time == lat.num_frames)
    if lat.reached_final:
        ends &= np.isfinite(lat.graph.final[lat.state])
    start = int(np.nonzero((lat.time == 0) & (lat.state == lat.graph.start))[0][0])
    found = []

    def walk(v, arcs):
        if ends[v]:
            found.append(tuple(arcs))
        for j in out_arcs[v]:
            walk(int(lat.dst[j]), arcs + [int(lat.arc[j])])

    walk(start, [])
    return found


@pytest.mark.parametrize('name', sorted(TOYS))
def test_full_beam_lattice_against_enumeration(name):
    """beam = inf.  Completeness: every enumerated path within lattice_beam of the best lies in the
    lattice.  Soundness: every lattice arc lies on such a path.  nbest: the enumerator's cheapest
    distinct word sequences under (cost, words).  Pruning is by arc, so two kept arcs of different
    good paths may join into a path beyond the lattice beam: the lattice's word sequences within
    best + lattice_beam are exactly the enumerator's, at exactly their costs (a cheaper alignment
    would lie within the beam, hence in the lattice); what nbest lists beyond that is a real path
    of the graph but need not be a sequence's cheapest.  So the comparison is exact up to
    best + lattice_beam, and over everything at lattice_beam = inf."""
    g, lp = toy_case(name)
    seen_paths, seen_seqs, tied = [], [], 0
    for scale in (1.0, 0.5):
        for lb in LATTICE_BEAMS:
            lats, _ = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF, lattice_beam=lb, acoustic_scale=scale)
            for b, n in enumerate(LENS):
                best, paths = LR.paths_within(R.graph_args(g), lp[:, b], n, lb, scale)
                lat = lats[b]
                assert float(lat.cost) == best
                in_lattice = set(_lattice_paths(lat))
                assert {p[1] for p in paths} <= in_lattice
                # soundness: the (time, arc) pairs of the lattice are those of the enumerated paths
                pairs = set()
                for _, arcs, _ in paths:
                    t = 0
                    for a in arcs:
                        pairs.add((t, a))
                        t += int(g.ilabel[a] > 0)
                assert {(int(lat.time[lat.src[j]]), int(lat.arc[j])) for j in range(lat.num_arcs)} == pairs
                want_all = LR.nbest_of(paths, 10 ** 6)
                if lb < INF:
                    seen_paths.append(len(paths))
                    seen_seqs.append(len(want_all))
                tied = max(tied, sum(1 for p in paths if p[0] == best))
                for k in (1, 3, 10, len(want_all) + 5):
                    got = lat.nbest(k)
                    inside = [e for e in got if e[1] <= best + lb]
                    # all of them, unless k cheaper ones came first
                    assert inside == want_all[:k] or (len(got) == k and inside == want_all[:len(inside)]), \
                        (name, scale, lb, b, k)
                    assert len(inside) == min(k, len(want_all)) or len(got) == k
                    if lb == INF:
                        assert got == want_all[:k]
                    assert got == sorted(got, key=lambda e: (e[1], e[0])) and lat.sentences(k) == [w for w, _ in got]
    # the finite lattice beams hold from one path up to hundreds (toy a: 737 paths, toy c: a handful)
    assert min(seen_paths) >= 1 and max(seen_paths) >= 8 and max(seen_seqs) >= 4, (seen_paths, seen_seqs)
    if name == 'b':
        assert tied >= 3         # several paths tie at the best cost: all of them are in the lattice
    if name in 'bc':        # utterance 1 (one frame) reaches no final state: the allow_partial case
        lat = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF)[0][1]
        assert not lat.reached_final and np.isfinite(lat.cost) and lat.beta[lat.time == 1].max() == 0


@pytest.mark.parametrize('name', sorted(TOYS))
def test_best_path_equals_decode_graph(name):
    g, lp = toy_case(name)
    x = torch.from_numpy(lp)
    for scale in (1.0, 0.5):
        for beam in (INF, 1.0):
            want = decode_graph(x, LENS, g, beam=beam, acoustic_scale=scale)
            for lb in LATTICE_BEAMS:
                lats, _ = decode_lattice(x, LENS, g, beam=beam, lattice_beam=lb, acoustic_scale=scale)
                assert best_paths(lats) == [lat.best_path() for lat in lats]        # one programme for all
                for b, lat in enumerate(lats):
                    words, cost, gc, ac = lat.best_path()
                    assert words == want['words'][b] and cost == float(want['cost'][b]), (name, scale, beam, lb, b)
                    assert cost == gc + scale * ac
                    assert lat.nbest(1)[0] == (words, cost) or lat.nbest(1)[0][1] == cost
    # one search, every scale: at lattice_beam = inf the lattice holds what any scale would pick
    lats, _ = decode_lattice(x, LENS, g, beam=INF, lattice_beam=INF, acoustic_scale=1.0)
    for scale in (0.5, 0.25, 2.0):
        want = decode_graph(x, LENS, g, beam=INF, acoustic_scale=scale)
        for b, lat in enumerate(lats):
            words, cost, _, _ = lat.best_path(acoustic_scale=scale)
            assert words == want['words'][b] and cost == float(want['cost'][b]), (name, scale, b)


def test_lm_scale_scales_graph_and_final_costs():
    g, lp = toy_case('a')
    lat = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF, lattice_beam=INF)[0][0]
    best, paths = LR.paths_within(R.graph_args(g), lp[:, 0], 5, INF)
    want = INF
    for _, arcs, _ in paths:
        t, c = 0, 0.0
        for a in arcs:
            c += 2.0 * float(g.weight[a])
            if g.ilabel[a] > 0:
                c -= 0.5 * float(lp[t, 0, g.ilabel[a] - 1])
                t += 1
        want = min(want, c + 2.0 * float(g.final[g.dst[arcs[-1]]]))
    words, cost, gc, ac = lat.best_path(acoustic_scale=0.5, lm_scale=2.0)
    assert cost == want == 2.0 * gc + 0.5 * ac
    assert lat.nbest(1, acoustic_scale=0.5, lm_scale=2.0)[0][1] == want


def test_no_final_state_without_allow_partial():
    g, lp = toy_case('c')
    lats, _ = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF, allow_partial=False)
    want = LR.lattices(R.graph_args(g), lp, LENS, beam=INF, allow_partial=False)
    for b in range(4):
        LR.assert_same(lats[b], want[b], b)
    assert lats[1].num_nodes == 0 and lats[1].num_arcs == 0 and np.isinf(lats[1].cost)
    assert lats[1].best_path() == ([], INF, INF, INF) and lats[1].nbest(3) == []


def test_refusals():
    g, lp = toy_case('a')
    x = torch.from_numpy(lp)
    with pytest.raises(ValueError):
        decode_lattice(x[0], LENS, g)
    with pytest.raises(ValueError):
        decode_lattice(x[:, :, :2], LENS, g)            # the graph reads class 2
    with pytest.raises(ValueError):
        decode_lattice(x, LENS, g, beam=-1.0)
    with pytest.raises(ValueError):
        decode_lattice(x, LENS, g, lattice_beam=-0.5)
    with pytest.raises(ValueError):
        decode_lattice(x, LENS, g, lattice_beam=float('nan'))
    with pytest.raises(ValueError):
        decode_lattice(x, LENS[:3], g)
    with pytest.raises(ValueError):
        decode_lattice(x, [5, 0, 3, 5], g)
    with pytest.raises(ValueError):
        decode_lattice(x, [6, 1, 3, 5], g)


def test_max_expansions_raises():
    g, lp = toy_case('a')
    lat = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF, lattice_beam=INF)[0][0]
    assert len(lat.nbest(10)) == 10
    with pytest.raises(RuntimeError, match='max_expansions'):
        lat.nbest(10, max_expansions=5)


def test_fst_decoder_nbest_on_the_shipped_bigram_lm():
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    kw = dict(normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab)
    torch.manual_seed(0)
    beamed = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), decode_beam=16.0, **kw)
    lattice = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), decode_beam=16.0,
                         decode_lattice_beam=4.0, decode_nbest=5, **kw)
    assert beamed.decode_lattice_beam is None and lattice.decode_nbest == 5
    lattice.load_state_dict(beamed.state_dict())
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    with torch.no_grad():
        want = beamed.decode(enc, elens)
        got = lattice.decode(enc, elens)
    assert 'nbest' not in want and got['decoded'] == want['decoded']
    for b in range(B):
        nb = got['nbest'][b]
        assert 1 <= len(nb) <= 5 and nb[0][0] == want['decoded'][b]
        costs = [c for _, c in nb]
        assert costs == sorted(costs) and costs[-1] <= costs[0] + 4.0 + 1e-3
        assert len({tuple(w) for w, _ in nb}) == len(nb)
    assert max(len(nb) for nb in got['nbest']) > 1


def test_tool_lattice_modes(tmp_path):
    """tools/decode_graph.py --lattice-beam --nbest, and --acwt-sweep: one search, 1-best per scale"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import decode_graph as tool
    finally:
        sys.path.pop(0)
    g, lp = toy_case('a')
    utts = [('utt%d' % b, lp[:n, b]) for b, n in enumerate(LENS)]
    out = tmp_path / 'nbest.txt'
    tool.write_nbest(g, utts, str(out), beam=INF, lattice_beam=2.0, nbest=3, acoustic_scale=1.0)
    lines = out.read_text().splitlines()
    lats, _ = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF, lattice_beam=2.0)
    want = []
    for b, lat in enumerate(lats):
        for k, (words, cost) in enumerate(lat.nbest(3)):
            want.append(' '.join(['utt%d-%d' % (b, k + 1), '%.6f' % cost] + [str(w) for w in words]))
    assert lines == want and len(lines) > 4
    sweep = tmp_path / 'sweep.txt'
    tool.write_sweep(g, utts, str(sweep), beam=INF, lattice_beam=INF, scales=tool.parse_sweep('0.5:1.0:0.25'))
    got = sweep.read_text().splitlines()
    want = []
    for scale in (0.5, 0.75, 1.0):
        ref = decode_graph(torch.from_numpy(lp), LENS, g, beam=INF, acoustic_scale=scale)
        for b in range(4):
            want.append(' '.join(['%g' % scale, 'utt%d' % b, '%.6f' % float(ref['cost'][b])] +
                                 [str(w) for w in ref['words'][b]]))
    assert got == want
