"""asr_wfst_lattice_f32 (csrc/wfst_lattice.hip) through att_speech.wfst_lattice.decode_lattice.

Inputs sit on the 2^-8 grid of tests/wfst_cases.py: every fp32 sum is exact, so the device must
equal the dense fp64 referee (tests/wfst_lattice_referee.py) in every canonical field, bit for
bit, with nothing redone on the host.  Frames beyond an utterance's length are NaN."""
import warnings

import numpy as np
import pytest
import torch

import wfst_lattice_referee as LR
import wfst_referee as R
from test_lattice_gpu import dev
from wfst_cases import INF, TOYS, assert_same, grid_scores, random_graph, toy_graph

from att_speech import wfst_lattice
from att_speech._native import lib
from att_speech.wfst_decode import DecodingGraph, decode_graph
from att_speech.wfst_lattice import decode_lattice

pytestmark = pytest.mark.gpu


def _device(g, lp, lens, **kw):
    return decode_lattice(torch.from_numpy(lp).to(dev()), lens, g, **kw)


def _check(g, lp, lens, **kw):
    lats, redone = _device(g, lp, lens, **kw)
    assert redone == []
    want = LR.lattices(R.graph_args(g), lp, lens, **kw)
    for b in range(len(lens)):
        LR.assert_same(lats[b], want[b], (kw, b))
    return lats, want


def test_the_entry_point_is_exported():
    L = lib()
    assert L.asr_wfst_lattice_supported(7, 16, 3, 5) == 1 and L.asr_wfst_lattice_supported(7, 16, 4097, 5) == 0
    assert L.asr_wfst_lattice_workspace_bytes(7, 2, 5, 7, 42) >= 2 * (12 * 7 + 20 * 7 + 24 * 42 + 8 * 7)
    assert L.asr_abi_version() == 24


@pytest.mark.parametrize('name', sorted(TOYS))
def test_toy_graphs(name):
    """lens 1 beside lens T in one batch; utterance 1 of toys b and c reaches no final state"""
    g = toy_graph(name)
    lens = [5, 1, 3, 5]
    lp = grid_scores(np.random.default_rng(len(name) + 3), 5, 4, 3, lens, low=-4.0)
    for scale in (1.0, 0.5):
        for beam in (INF, 1.0):
            for lb in (0.0, 1.0, 2.0, 4.0, INF):
                _check(g, lp, lens, beam=beam, lattice_beam=lb, acoustic_scale=scale)


def test_fan_out_and_fan_in():
    """3000 out-arcs of one state and 3000 arcs into one state, most at equal cost: every tied arc
    is within lattice_beam = 0, whichever lane gets there first"""
    rng = np.random.default_rng(7)
    F, C = 3000, 5
    hub, sink, end = 0, F + 1, F + 2
    mid = np.arange(1, F + 1)
    src = np.concatenate([np.full(F, hub), mid, [sink, sink, hub, sink]])
    dst = np.concatenate([mid, np.full(F, sink), [hub, end, hub, sink]])
    il = np.concatenate([rng.integers(1, C + 1, F), rng.integers(1, 3, F), [1, 0, 2, 3]])
    ol = np.concatenate([rng.permutation(F) + 1, rng.permutation(F) + 5000, [0, 9001, 9002, 0]])
    w = np.concatenate([rng.integers(0, 2, F) / 4.0, np.zeros(F), [0.5, 0.25, 1.0, 0.75]])
    final = np.full(F + 3, INF)
    final[end] = 0.5
    final[5] = 0.0
    perm = rng.permutation(len(src))
    g = DecodingGraph(F + 3, 0, src[perm], dst[perm], il[perm], ol[perm], w[perm], final)
    lens = [4, 3]
    lp = -rng.integers(1, 3, size=(4, 2, C)).astype(np.float32)
    lp[3:, 1] = np.nan
    lats, _ = _check(g, lp, lens, beam=INF, lattice_beam=0.0)
    assert max(l.num_arcs for l in lats) > 200          # the ties are all there
    _check(g, lp, lens, beam=INF, lattice_beam=0.5)


def test_wide_state_ids():
    """70 000 states: ids beyond 16 bits, epsilon arcs at two ranks"""
    rng = np.random.default_rng(70)
    g = random_graph(rng, 70000, 50, arcs_per_state=4)
    assert g.num_ranks == 2
    lens = [12, 7, 12]
    lp = grid_scores(rng, 12, 3, 50, lens)
    lats, _ = _check(g, lp, lens, beam=INF, lattice_beam=2.0)
    assert max(int(l.state.max()) for l in lats) > 65535
    _check(g, lp, lens, beam=6.0, lattice_beam=2.0, acoustic_scale=0.5)


def test_wide_alphabet():
    rng = np.random.default_rng(2401)
    C = 2401
    g0 = random_graph(rng, 600, C, arcs_per_state=6)
    il = g0.ilabel.copy()
    il[g0.ptr[0]] = C                           # the start state reads the last class
    g = DecodingGraph(g0.num_states, 0, g0.src, g0.dst, il, g0.olabel, g0.weight, g0.final)
    lens = [8, 5]
    lp = grid_scores(rng, 8, 2, C, lens)
    lp[0, :, C - 1] = 0.0
    lats, _ = _check(g, lp, lens, beam=INF, lattice_beam=4.0)
    assert any((l.ilabel == C).any() for l in lats)
    _check(g, lp, lens, beam=4.0, lattice_beam=INF)


def test_pruned_source_of_a_negative_epsilon_arc():
    """state 1 reaches state 2 over an epsilon arc of weight -3: with beam = 1 the closure's own
    result prunes state 1 while state 2 survives, and the lattice must still hold the arc 1 -> 2"""
    arcs = [(0, 1, 11, 0.0, 1), (0, 2, 12, 0.5, 3), (1, 0, 13, -3.0, 2), (2, 1, 14, 0.25, 4), (2, 2, 0, 0.5, 0),
            (3, 1, 15, 0.0, 4), (4, 1, 0, 0.25, 1), (4, 2, 16, 0.0, 4), (1, 2, 0, 0.0, 4)]
    src, il, ol, w, dst = [np.array(x) for x in zip(*arcs)]
    final = np.full(5, INF)
    final[[2, 4]] = [0.25, 0.0]
    g = DecodingGraph(5, 0, src, dst, il, ol, w, final)
    lens = [4, 2, 3]
    lp = grid_scores(np.random.default_rng(5), 4, 3, 2, lens, low=-1.0)
    lats, want = _check(g, lp, lens, beam=1.0, lattice_beam=INF)
    hit = 0
    for lat in lats:
        for j in np.nonzero(lat.arc == int(np.nonzero((g.src == 1) & (g.ilabel == 0))[0][0]))[0]:
            at = lat.time == lat.time[lat.src[j]]
            hit += lat.alpha[lat.src[j]] > lat.alpha[at].min() + 1.0        # the source did not survive
    assert hit > 0
    _check(g, lp, lens, beam=1.0, lattice_beam=0.5)


def test_finite_beam_changes_the_lattice():
    """Seeds picked on the CPU (host path) so that beam = 2 loses arcs the full search keeps."""
    picked = None
    for seed in range(40):
        rng = np.random.default_rng(seed)
        g = random_graph(rng, 400, 9, final_share=0.05)
        lens = [14, 9, 14]
        lp = grid_scores(rng, 14, 3, 9, lens)
        full = LR.lattices(R.graph_args(g), lp, lens, beam=INF, lattice_beam=4.0)
        tight = LR.lattices(R.graph_args(g), lp, lens, beam=2.0, lattice_beam=4.0)
        if any(len(a['arc']) != len(b['arc']) for a, b in zip(full, tight)) and \
                any(a['cost'] != b['cost'] for a, b in zip(full, tight)):
            picked = (g, lp, lens, tight)
            break
    assert picked is not None
    g, lp, lens, tight = picked
    lats, redone = _device(g, lp, lens, beam=2.0, lattice_beam=4.0)
    assert redone == []
    for b in range(3):
        LR.assert_same(lats[b], tight[b], b)
    _check(g, lp, lens, beam=0.0, lattice_beam=4.0)
    _check(g, lp, lens, beam=16.0, lattice_beam=1.0)


@pytest.mark.parametrize('allow_partial', [True, False])
def test_no_final_state_reached(allow_partial):
    g = toy_graph('c')                          # its final state is at least three frames away
    lens = [1, 2, 2]
    lp = grid_scores(np.random.default_rng(4), 2, 3, 3, lens, low=-4.0)
    lats, want = _check(g, lp, lens, beam=INF, lattice_beam=2.0, allow_partial=allow_partial)
    assert not any(l.reached_final for l in lats)
    if allow_partial:
        assert all(np.isfinite(l.cost) and l.num_arcs >= l.num_frames for l in lats)
    else:
        assert all(np.isinf(l.cost) and l.num_nodes == 0 and l.num_arcs == 0 for l in lats)


def _redo_case(monkeypatch, g, lp, lens, beam, lb, caps, exceeded):
    """Run with the given capacities (the plan of the workspace is replaced, nothing else).  Host
    statistics say what utterance 1, and only that one, outgrows: `exceeded` names the capacities.
    It must come back flagged, be redone on the host with one warning, and equal the referee."""
    list_cap, log_cap, node_cap, arc_cap = caps
    stats = wfst_lattice.decode_lattice_host(np.nan_to_num(lp), lens, g, beam=beam, lattice_beam=lb)[1]
    over = [dict(list=max(s['peak_emit'], s['peak_closure']) > list_cap, log=s['records'] > log_cap,
                 nodes=s['nodes'] > node_cap, arcs=s['arcs'] > arc_cap) for s in stats]
    assert not any(over[0].values()) and not any(over[2].values()), (over, stats)
    assert {k for k, v in over[1].items() if v} == set(exceeded.split('+')), (over, stats)
    monkeypatch.setattr(wfst_lattice, 'plan_workspace',
                        lambda N, T, B, budget, A=None: (B, list_cap, log_cap, node_cap, arc_cap))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        lats, redone = _device(g, lp, lens, beam=beam, lattice_beam=lb)
    msgs = [str(w.message) for w in rec if 'decode_lattice' in str(w.message)]
    assert len(msgs) == 1 and exceeded.split('+')[0] in msgs[0]
    assert redone == [1]
    want = LR.lattices(R.graph_args(g), lp, lens, beam=beam, lattice_beam=lb)
    for b in range(3):
        LR.assert_same(lats[b], want[b], b)


def _redo_inputs():
    rng = np.random.default_rng(12)
    g = random_graph(rng, 300, 11)
    lens = [3, 16, 3]
    return g, grid_scores(rng, 16, 3, 11, lens), lens


def test_list_overflow(monkeypatch):
    g, lp, lens = _redo_inputs()
    _redo_case(monkeypatch, g, lp, lens, INF, 2.0, (150, 17 * 300, 17 * 300, 17 * 1200), 'list')


def test_log_overflow(monkeypatch):
    g, lp, lens = _redo_inputs()
    _redo_case(monkeypatch, g, lp, lens, INF, 2.0, (300, 1500, 17 * 300, 17 * 1200), 'log')


def test_node_overflow(monkeypatch):
    g, lp, lens = _redo_inputs()
    stats = wfst_lattice.decode_lattice_host(np.nan_to_num(lp), lens, g, beam=INF, lattice_beam=2.0)[1]
    cap = max(stats[0]['nodes'], stats[2]['nodes'])
    _redo_case(monkeypatch, g, lp, lens, INF, 2.0, (300, 17 * 300, cap, 17 * 1200), 'nodes')


def test_arc_overflow(monkeypatch):
    g, lp, lens = _redo_inputs()
    stats = wfst_lattice.decode_lattice_host(np.nan_to_num(lp), lens, g, beam=INF, lattice_beam=2.0)[1]
    cap = max(stats[0]['arcs'], stats[2]['arcs'])
    _redo_case(monkeypatch, g, lp, lens, INF, 2.0, (300, 17 * 300, 17 * 300, cap), 'arcs')


def test_tables_beyond_the_budget_run_in_chunks():
    rng = np.random.default_rng(13)
    g = random_graph(rng, 5000, 11)
    lens = [6, 4, 6, 5, 6]
    lp = grid_scores(rng, 6, 5, 11, lens)
    # three quarters of the budget are the search's; the tables of two utterances take half of that
    budget = 16 * (12 * 5000 + 8 * 8) // 3 + 4096
    assert wfst_lattice.plan_workspace(5000, 6, 5, budget, len(g.src))[0] == 2
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        lats, _ = _device(g, lp, lens, beam=3.0, lattice_beam=2.0, workspace_bytes=budget)
    want = LR.lattices(R.graph_args(g), lp, lens, beam=3.0, lattice_beam=2.0)
    for b in range(5):
        LR.assert_same(lats[b], want[b], b)


def test_switch_selects_the_host_path_per_call(monkeypatch):
    from att_speech import _native
    g = toy_graph('a')
    lens = [5, 1, 3, 5]
    lp = grid_scores(np.random.default_rng(9), 5, 4, 3, lens, low=-4.0)
    native, _ = _device(g, lp, lens, beam=2.0, lattice_beam=2.0)
    monkeypatch.setenv('ASR_WFST_LATTICE_NATIVE', '0')
    monkeypatch.setattr(_native, 'lib', lambda: pytest.fail('the native library was called'))
    host, _ = _device(g, lp, lens, beam=2.0, lattice_beam=2.0)
    for a, b in zip(native, host):
        for k in a.FIELDS:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_more_than_4096_classes_are_refused():
    g = toy_graph('a')
    lp = torch.zeros(2, 1, 4097, device=dev())
    with pytest.raises(NotImplementedError):
        decode_lattice(lp, [2], g)


def test_unquantised_scores_match_the_host_path_bit_for_bit():
    rng = np.random.default_rng(40)
    g0 = random_graph(rng, 3000, 40, arcs_per_state=5)
    w = rng.standard_normal(len(g0.src)).astype(np.float32) + np.float32(0.7)
    fin = np.where(np.isfinite(g0.final), rng.random(g0.num_states).astype(np.float32), np.float32(INF))
    g = DecodingGraph(g0.num_states, 0, g0.src, g0.dst, g0.ilabel, g0.olabel, w, fin)
    T, B = 40, 8
    lens = rng.integers(T // 2, T + 1, size=B)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, B, 40)).astype(np.float32) * 3), -1)
    for scale, lb in ((1.0, 0.0), (0.3, 3.0)):
        got, redone = decode_lattice(lp.to(dev()), lens, g, beam=16.0, lattice_beam=lb, acoustic_scale=scale)
        want, _ = decode_lattice(lp, lens, g, beam=16.0, lattice_beam=lb, acoustic_scale=scale)
        assert redone == []
        for a, b in zip(got, want):
            assert a.num_arcs >= a.num_frames and a.reached_final == b.reached_final
            assert np.float32(a.cost).view(np.int32) == np.float32(b.cost).view(np.int32)
            for k in ('time', 'state', 'src', 'dst', 'arc'):
                assert np.array_equal(getattr(a, k), getattr(b, k)), k
            for k in ('alpha', 'beta', 'lp'):
                assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), k


def test_decode_graph_still_equals_its_referee():
    """the 1-best search shares its device code with the lattice kernel: same session, same bits"""
    g = toy_graph('a')
    lens = [5, 1, 3, 5]
    lp = grid_scores(np.random.default_rng(4), 5, 4, 3, lens, low=-4.0)
    _device(g, lp, lens, beam=1.0, lattice_beam=1.0)
    for beam in (INF, 1.0):
        got = decode_graph(torch.from_numpy(lp).to(dev()), lens, g, beam=beam)
        assert got['redone_on_host'] == []
        assert_same(got, R.decode(*R.graph_args(g), lp, lens, beam=beam), str(beam))
