"""att_speech.wfst_decode on the CPU: the host path against the fp64 referee
(tests/wfst_referee.py) and a brute-force enumeration of all paths, graph validation, the
workspace plan and the command-line tool.  Inputs sit on the 2^-8 grid of tests/wfst_cases.py,
so every comparison is ==."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wfst_referee as R
from conftest import ROOT
from wfst_cases import INF, TOYS, assert_same, grid_scores, random_graph, toy_graph


def _host(g, lp, lens, **kw):
    from att_speech.wfst_decode import decode_graph
    return decode_graph(torch.from_numpy(lp), lens, g, **kw)


@pytest.mark.parametrize('name', sorted(TOYS))
@pytest.mark.parametrize('T', [1, 2, 5])
@pytest.mark.parametrize('scale', [1.0, 0.5])
def test_host_path_matches_referee_and_enumeration(name, T, scale):
    g = toy_graph(name)
    assert 5 <= g.num_states <= 8
    rng = np.random.default_rng(T * 10 + len(name))
    B = 6
    lens = [T] * B
    lp = grid_scores(rng, T, B, 3, low=-4.0)
    got = _host(g, lp, lens, beam=INF, acoustic_scale=scale)
    want = R.decode(*R.graph_args(g), lp, lens, beam=INF, acoustic_scale=scale)
    assert_same(got, want, name)
    assert got['redone_on_host'] == []
    for b in range(B):
        paths = R.enumerate_paths(*R.graph_args(g), lp[:, b], T, scale)
        final = [p for p in paths if p[0] < INF]
        if final:
            best = min(p[0] for p in final)
            assert bool(got['reached_final'][b])
        else:
            best = min(p[1] for p in paths)
            assert not bool(got['reached_final'][b])
        assert float(got['cost'][b]) == best
        # the returned path is one of the enumerated optima: same words, same alignment
        optima = [p for p in (final or paths) if (p[0] if final else p[1]) == best]
        sig = {(tuple(int(g.olabel[a]) for a in p[2] if g.olabel[a] != 0),
                tuple(int(g.ilabel[a]) for a in p[2] if g.ilabel[a] > 0)) for p in optima}
        assert (tuple(got['words'][b]), tuple(got['alignment'][b, :T].tolist())) in sig


def test_toy_graphs_have_the_features_the_tests_are_about():
    g = toy_graph('a')
    assert g.num_ranks == 3 and (g.weight[g.ilabel == 0] < 0).any()           # chain three deep, negative
    assert (g.olabel[g.ilabel == 0] != 0).any() and (g.olabel[g.ilabel > 0] != 0).any()
    # arcs keep their input order inside a source: the tie between the two parallel arcs of toy b
    gb = toy_graph('b')
    first = gb.ptr[0]
    assert gb.olabel[first] == 1 and gb.olabel[first + 1] == 2
    lp = np.zeros((1, 1, 3), np.float32)
    lp[0, 0, 1:] = -8.0
    assert _host(gb, lp, [1], beam=INF)['words'] == [[1]]


@pytest.mark.parametrize('beam', [0.0, 1.0, 2.0, 16.0])
def test_host_path_matches_referee_under_a_beam(beam):
    rng = np.random.default_rng(int(beam * 4) + 1)
    lens = [7, 1, 4, 7]
    for name in sorted(TOYS):
        lp = grid_scores(rng, 7, 4, 3, lens, low=-4.0)
        g = toy_graph(name)
        for partial in (True, False):
            assert_same(_host(g, lp, lens, beam=beam, allow_partial=partial),
                        R.decode(*R.graph_args(g), lp, lens, beam=beam, allow_partial=partial), name)
    g = random_graph(rng, 300, 11)
    assert g.num_ranks == 2
    lp = grid_scores(rng, 7, 4, 11, lens)
    got = _host(g, lp, lens, beam=beam, acoustic_scale=0.5)
    assert_same(got, R.decode(*R.graph_args(g), lp, lens, beam=beam, acoustic_scale=0.5))


def test_beam_prunes_and_changes_the_answer_somewhere():
    """a finite beam is not a no-op: over a few seeds it removes tokens and changes a result"""
    pruned = changed = 0
    for seed in range(12):
        rng = np.random.default_rng(seed)
        g = random_graph(rng, 200, 7, final_share=0.05)
        lp = grid_scores(rng, 10, 2, 7)
        full = _host(g, lp, [10, 10], beam=INF)
        tight = _host(g, lp, [10, 10], beam=2.0)
        pruned += int((tight['num_active'] < full['num_active']).any())
        changed += int((tight['cost'] != full['cost']).any())
    assert pruned and changed


def test_epsilon_cycle_is_refused():
    from att_speech.wfst_decode import DecodingGraph
    with pytest.raises(ValueError, match='cycle'):
        DecodingGraph(3, 0, [0, 1, 2, 0], [1, 2, 1, 2], [1, 0, 0, 2], [0, 0, 0, 0], [0.0, 0.5, 0.5, 1.0],
                      [INF, INF, 0.0])
    with pytest.raises(ValueError, match='cycle'):          # an epsilon self-loop
        DecodingGraph(2, 0, [0, 1], [1, 1], [1, 0], [0, 0], [0.0, 0.0], [INF, 0.0])
    with pytest.raises(ValueError, match='finite'):
        DecodingGraph(2, 0, [0], [1], [1], [0], [INF], [INF, 0.0])


def test_ilabels_are_checked_against_the_class_count():
    g = toy_graph('a')                                       # reads classes 0..2
    with pytest.raises(ValueError, match='class'):
        _host(g, np.zeros((2, 1, 2), np.float32), [2])
    _host(g, np.zeros((2, 1, 3), np.float32), [2])
    with pytest.raises(ValueError, match='lens'):
        _host(g, np.zeros((2, 1, 3), np.float32), [3])


def test_readers_and_graph_generator(tmp_path):
    """AT&T text and OpenFst binary through lm_fst; HC o G of a generator against the referee"""
    from att_speech.lm_fst import LmFst
    from att_speech.wfst_decode import DecodingGraph
    from att_speech import fst_utils as P
    from grammar_cases import toy_lm
    g = toy_graph('a')
    txt = tmp_path / 'g.txt'
    with open(txt, 'w') as f:
        for a in range(len(g.src)):
            f.write('%d %d %d %d %r\n' % (g.src[a], g.dst[a], g.ilabel[a], g.olabel[a], float(g.weight[a])))
        for s in np.nonzero(np.isfinite(g.final))[0]:
            f.write('%d %r\n' % (s, float(g.final[s])))
    g_txt = DecodingGraph.read(str(txt))
    LmFst.read(str(txt)).write(str(tmp_path / 'g.fst'))
    g_bin = DecodingGraph.read(str(tmp_path / 'g.fst'))
    rng = np.random.default_rng(5)
    lp = grid_scores(rng, 5, 3, 3, low=-4.0)
    full = _host(g, lp, [5, 5, 5], beam=INF)
    for other in (g_txt, g_bin):                             # lm_fst sorts a source's arcs by ilabel: other
        assert len(other.src) == len(g.src)                  # arc indices, the same best costs
        got = _host(other, lp, [5, 5, 5], beam=INF)
        assert (got['cost'] == full['cost']).all() and np.isfinite(full['cost'].numpy()).all()
        assert_same(got, R.decode(*R.graph_args(other), lp, [5, 5, 5], beam=INF))

    lm, vocab = toy_lm('s4')
    gg = P.CTCGraphGen(context_order=1, num_symbols=4, grammar_fst=lm, vocabulary=vocab)
    dg = DecodingGraph.from_graph_generator(gg)
    assert dg.num_states == gg.grammar.num_states and dg.num_ranks == 0
    x = rng.standard_normal((6, 2, 4)).astype(np.float32)
    got = _host(dg, x, [6, 4], beam=INF)
    ref = R.decode(*R.graph_args(dg), x, [6, 4], beam=INF)
    assert got['words'] == ref['words'] and (got['alignment'].numpy() == ref['alignment']).all()
    np.testing.assert_allclose(got['cost'].numpy(), ref['cost'], rtol=1e-5)
    for b, n in enumerate([6, 4]):                           # the words are HC's read-out of the alignment
        assert got['words'][b] == gg.decoding_fst.read_out(got['alignment'][b, :n].numpy() - 1)
    hc = DecodingGraph.from_graph_generator(P.CTCGraphGen(context_order=2, num_symbols=3))
    assert hc.num_states == 9 and hc.max_ilabel == 9 and np.isfinite(hc.final).all()


def test_workspace_plan():
    from att_speech.wfst_decode import plan_workspace
    from att_speech import _native
    L = _native.lib()
    for N, T, B, budget in [(7, 5, 4, 1 << 20), (70000, 12, 3, 8 << 20), (1000000, 334, 16, 64 << 20),
                            (194, 334, 768, 256 << 20), (50, 12, 3, 4000)]:
        chunk, list_cap, log_cap = plan_workspace(N, T, B, budget)
        assert 1 <= chunk <= B and 1 <= list_cap <= N and 1 <= log_cap <= (T + 1) * list_cap
        assert 0 < L.asr_wfst_decode_workspace_bytes(N, chunk, list_cap, log_cap) <= budget
    assert plan_workspace(1000000, 334, 16, 64 << 20)[0] < 16            # the batch is split
    with pytest.raises(ValueError):
        plan_workspace(1000, 5, 1, 12000)
    # a share per utterance just above its tables: fewer utterances a launch, never a plan that does not fit
    for budget in range(12 * 40 * 100, 12 * 40 * 100 + 40000, 997):
        chunk, list_cap, log_cap = plan_workspace(40, 300, 100, budget)
        assert 0 < L.asr_wfst_decode_workspace_bytes(40, chunk, list_cap, log_cap) <= budget
    assert L.asr_wfst_decode_supported(70000, 280000, 2401, 8) == 1
    assert L.asr_wfst_decode_supported(70000, 280000, 5000, 8) == 0


def test_decode_graph_tool_round_trip(tmp_path):
    """archive + graph file + words.txt -> one `uttid w1 w2 ...` line per utterance"""
    from att_speech.ctc_forward import KaldiFloatMatrixWriter
    g = toy_graph('a')
    rng = np.random.default_rng(11)
    lens = [5, 2, 4]
    lp = grid_scores(rng, 5, 3, 3, low=-4.0)
    with KaldiFloatMatrixWriter('ark:' + str(tmp_path / 'lp.ark')) as w:
        for b, n in enumerate(lens):
            w['utt%d' % b] = lp[:n, b]
    with open(tmp_path / 'g.txt', 'w') as f:
        for a in range(len(g.src)):
            f.write('%d %d %d %d %r\n' % (g.src[a], g.dst[a], g.ilabel[a], g.olabel[a], float(g.weight[a])))
        for s in np.nonzero(np.isfinite(g.final))[0]:
            f.write('%d %r\n' % (s, float(g.final[s])))
    with open(tmp_path / 'words.txt', 'w') as f:
        f.write('<eps> 0\n')
        for k in range(1, 10):
            f.write('w%d %d\n' % (k, k))
    from att_speech.wfst_decode import DecodingGraph
    want = _host(DecodingGraph.read(str(tmp_path / 'g.txt')), np.nan_to_num(lp), lens, beam=8.0,
                 acoustic_scale=0.5)
    tool = os.path.join(ROOT, 'tools', 'decode_graph.py')
    for extra, fmt in ((['--words', str(tmp_path / 'words.txt')], 'w%d'), ([], '%d')):
        out = tmp_path / 'hyp.txt'
        subprocess.check_call([sys.executable, tool, str(tmp_path / 'lp.ark'), str(tmp_path / 'g.txt'),
                               '--beam', '8', '--acoustic-scale', '0.5', '--batch', '2', '--device', 'cpu',
                               '--out', str(out)] + extra)
        lines = open(out).read().splitlines()
        assert lines == [' '.join(['utt%d' % b] + [fmt % w for w in want['words'][b]]) for b in range(3)]
    assert any(want['words'])
