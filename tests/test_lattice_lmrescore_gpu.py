"""asr_lattice_lmrescore_expand / _emit / _sweep (csrc/lattice_lm.hip) through DeviceLatticeBatch.rescore_lm:
the device path equals the numpy twin of att_speech.lattice_lm bit for bit (every lattice field, the stats and
every array of the RescoredGraph), with no utterance redone on the host and no warning, over the cases of
tests/test_lattice_lmrescore.py and the shapes at which the kernels take another path.  Then the consumers
(best_paths, nbest, posteriors, mbr) on the rescored batch against their twins."""
import warnings

import numpy as np
import pytest
import torch

import lm_rescore_cases as RC
import mbr_cases as MC
from lm_rescore_cases import INF

from att_speech import lattice_lm
from att_speech.lattice_dp import DeviceLatticeBatch
from att_speech.lattice_lm import BackoffLm
from att_speech.wfst_lattice import Lattice, LatticeBatch, _empty

pytestmark = pytest.mark.gpu

GRAPH_FIELDS = ('src', 'dst', 'ilabel', 'olabel', 'weight', 'final', 'ptr', 'rank', 'state_pairs', 'arc_base',
                'arc_lm_state', 'arc_lm_cost')


def dev():
    return torch.device('cuda:0')


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_same(got, want, what, stats=True):
    """got: a DeviceLatticeBatch, want: the twin's LatticeBatch"""
    assert got.device.type == 'cuda'
    lats = got.lattices()
    assert len(lats) == len(want.lattices)
    for b, (x, y) in enumerate(zip(lats, want.lattices)):
        for f in Lattice.FIELDS:
            a, c = getattr(x, f), getattr(y, f)
            assert a.dtype == c.dtype and a.shape == c.shape and bits(a) == bits(c), (what, b, f)
        assert bits(x.cost) == bits(y.cost) and x.reached_final == y.reached_final, (what, b)
        assert x.num_frames == y.num_frames and x.acoustic_scale == y.acoustic_scale, (what, b)
    gx, gy = got.graph, want.lattices[0].graph if want.lattices else None
    if gy is not None:
        assert gx.num_states == gy.num_states and gx.start == gy.start, what
        for f in GRAPH_FIELDS:
            a, c = getattr(gx, f), getattr(gy, f)
            assert a.dtype == c.dtype and a.shape == c.shape and bits(a) == bits(c), (what, 'graph', f)
    if stats:
        assert got.stats == want.stats, (what, got.stats, want.stats)


def both(lats, lm, what, **kw):
    """rescore on the device without a warning and on the host; assert equality; return both"""
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
        got = batch.rescore_lm(lm, **kw)
    kw.pop('workspace_bytes', None)
    want = LatticeBatch(lats).rescore_lm(lm, graph=lats[0].graph, **kw)
    assert got.stats['redone_on_host'] == []
    assert_same(got, want, what)
    return got, want


@pytest.mark.parametrize('k', range(len(RC.BRUTE)))
def test_brute_cases(k):
    _, lats, lm = RC.brute_case(k)                      # k = 2: partial utterances (reached_final False)
    for scale in (1.0, 0.5, -1.0):
        for lb in (None, 1.0, 0.0):
            got, _ = both(lats, lm, 'brute %d %s %s' % (k, scale, lb), scale=scale, lattice_beam=lb)
    assert got.num_nodes > 0
    if k == 2:
        assert not any(l.reached_final for l in lats)


def test_shipped_lms_and_cap():
    _, lats, tg, lmap = RC.shipped_case()
    blm = BackoffLm.from_fst(tg)
    got, want = both(lats, blm, 'shipped', label_map=lmap)
    top = want.stats['max_lm_states']
    assert 1 < top < lattice_lm.DEFAULT_MAX_LM_STATES
    both(lats, blm, 'shipped, beam', label_map=lmap, lattice_beam=2.0)
    # a node's list reaches exactly the cap
    both(lats, blm, 'cap reached', label_map=lmap, max_lm_states=top)
    # cap plus one: that utterance is redone by the twin, one warning, the same result; the others stay
    batch = DeviceLatticeBatch.from_lattices(lats, dev())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        over = batch.rescore_lm(blm, label_map=lmap, max_lm_states=top - 1)
    assert len(caught) == 1 and 'max_lm_states' in str(caught[0].message)
    redone = over.stats['redone_on_host']
    assert 1 <= len(redone) < len(lats)
    per = [LatticeBatch([l]).rescore_lm(blm, label_map=lmap).stats['max_lm_states'] for l in lats]
    assert redone == [b for b, n in enumerate(per) if n > top - 1]
    assert_same(over, want, 'cap plus one', stats=False)
    assert dict(over.stats, redone_on_host=[]) == want.stats
    # small workspace_bytes: several launches, the same bits
    nodes = max(l.num_nodes for l in lats)
    small, _ = both(lats, blm, 'small workspace', label_map=lmap, workspace_bytes=4 * 256 * nodes + 128)
    assert small.launches >= 2 * len(lats) + 1 and got.launches == 3
    with pytest.raises(ValueError, match='workspace_bytes'):
        DeviceLatticeBatch.from_lattices(lats, dev()).rescore_lm(blm, label_map=lmap, workspace_bytes=4 * 256 * nodes + 100)
    # run to run
    again, _ = both(lats, blm, 'again', label_map=lmap)
    for f in Lattice.FIELDS:
        assert torch.equal(getattr(again, f), getattr(got, f)), f


def test_shapes():
    lm = RC.fan_lm()
    _, lats, blm_lm = RC.brute_case(0)
    # an empty lattice in the middle
    mixed = [lats[0], _empty(lats[0].graph, 1.0, 4), lats[1]]
    got, _ = both(mixed, blm_lm, 'empty in the middle')
    assert got.lattices()[1].num_nodes == 0 and got.cost[1] == np.float32(INF)
    # every level holds one node
    single = MC.single_path()
    got, _ = both([single], lm, 'single path')
    assert got.num_nodes == single.num_nodes
    # 255, 256 and 257 nodes in one utterance; the end node has more than 64 in-arcs
    for n in (255, 256, 257):
        lat = RC.fan(n)
        assert lat.num_nodes == n
        for lb in (None, 1.0):
            got, want = both([lat], lm, 'fan %d %s' % (n, lb), lattice_beam=lb)
        assert want.stats['max_lm_states'] > 4
    # all utterances die
    none = np.full(RC.N_WORDS + 1, -1)
    none[0] = 0
    got, _ = both([RC.fan(70)], lm, 'all die', label_map=none)
    assert got.num_nodes == 0 and got.num_arcs == 0
    # a finite out-of-vocabulary cost
    both(lats, blm_lm, 'oov cost', label_map=none, oov_cost=2.5)
    both(lats, blm_lm, 'oov cost, real map', oov_cost=1.25, scale=0.5)


def test_consumers():
    _, lats, tg, lmap = RC.shipped_case()
    got, want = both(lats, BackoffLm.from_fst(tg), 'shipped', label_map=lmap, lattice_beam=3.0)
    host = LatticeBatch(got.lattices())
    pairs = [(None, 1.0), (0.5, 1.0), (1.0, 0.8)]
    sweep = got.best_paths([a for a, _ in pairs], [l for _, l in pairs])
    for k, (a, l) in enumerate(pairs):
        assert sweep[k] == host.best_paths(a, l), (a, l)
    assert got.nbest(5) == host.nbest(5)
    assert got.sentences(3) == [[w for w, _ in row] for row in host.nbest(3)]
    post, ref = got.posteriors(), host.posteriors()
    for x, y in ((post.log_z, ref.log_z), (post.arc_log_post, ref.arc_log_post), (post.node_log_post, ref.node_log_post)):
        x = x.cpu().numpy()
        big = y > -30.0
        assert (np.abs(x[big] - y[big]) <= 1e-9).all()                      # tests/test_lattice_dp_gpu.py's TOL
        assert (np.abs(np.exp(x[~big]) - np.exp(y[~big])) <= 1e-12).all()
    for x, y in zip(got.mbr(), host.mbr()):
        assert (x.risk < INF) == (y.risk < INF)
        assert abs(x.risk - y.risk) <= 10 * 6.37e-12                        # tests/test_lattice_mbr_gpu.py's RISK_TOL


def test_twice_in_a_row():
    """bigram out, trigram in"""
    _, lats, tg, lmap = RC.shipped_case()
    bg, tg = BackoffLm.from_fst(RC.bigram_lm()), BackoffLm.from_fst(tg)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
        out = batch.rescore_lm(bg, label_map=lmap, scale=-1.0)
        back = out.rescore_lm(tg, label_map=lmap, scale=1.0, lattice_beam=4.0)
    h_out = LatticeBatch(lats).rescore_lm(bg, label_map=lmap, scale=-1.0)
    h_back = LatticeBatch(h_out.lattices).rescore_lm(tg, label_map=lmap, scale=1.0, lattice_beam=4.0)
    assert_same(out, h_out, 'bigram out')
    assert_same(back, h_back, 'trigram in')
    assert back.graph.base.base is lats[0].graph
    assert back.best_paths()[0] == h_back.best_paths()
