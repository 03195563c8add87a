"""att_speech.lattice_lm on the CPU: the numpy twin of lattice o back-off LM against brute force (every
complete path of tiny lattices, an independent LM scorer), its canonical form, pruning, out-of-vocabulary
words, malformed LMs and the C ABI's size entries.  The device path is held to this twin bit for bit in
tests/test_lattice_lmrescore_gpu.py."""
import warnings

import numpy as np
import pytest

import lm_rescore_cases as RC
from lm_rescore_cases import INF

from att_speech import _native, lattice_lm
from att_speech.lattice_dp import DeviceLatticeBatch
from att_speech.lattice_lm import BackoffLm, RescoredGraph
from att_speech.lm_fst import LmFst
from att_speech.wfst_lattice import Lattice, LatticeBatch, _empty

EVERY = 200000


def identity(lat):
    """a path's identity that survives the projection: (time and graph state of the source, graph arc) per arc"""
    def ident(path):
        return tuple((int(lat.time[lat.src[j]]), int(lat.state[lat.src[j]]), int(lat.arc[j])) for j in path)
    return ident


def projected(lat):
    g = lat.graph

    def ident(path):
        return tuple((int(lat.time[lat.src[j]]), int(g.state_pairs[lat.state[lat.src[j]], 0]),
                      int(g.arc_base[lat.arc[j]])) for j in path)
    return ident


def lm_cost(lm, lat, words):
    arcs, end = RC.score_words(lm, words)
    return arcs + end if lat.reached_final else arcs


@pytest.mark.parametrize('k', range(len(RC.BRUTE)))
@pytest.mark.parametrize('scale', [1.0, 0.5, -1.0])
def test_brute_force(k, scale):
    g, lats, lm = RC.brute_case(k)
    res = LatticeBatch(lats).rescore_lm(lm, scale=scale)
    assert isinstance(res.lattices[0].graph, RescoredGraph) and res.lattices[0].graph.base is g
    total = 0
    for b, (old, new) in enumerate(zip(lats, res.lattices)):
        assert new.graph is res.lattices[0].graph
        paths = RC.complete_paths(old)                      # raises beyond 20 000
        want = {}
        for p in paths:
            c = lm_cost(lm, old, RC.path_words(old, p))
            if c < INF:
                want[identity(old)(p)] = RC.path_graph_cost(old, p) + scale * c
        old_arc = {identity(old)((j,))[0]: j for j in range(old.num_arcs)}
        got_paths = RC.complete_paths(new)
        got = {projected(new)(p): p for p in got_paths}
        assert len(got) == len(got_paths), (b, 'the projection is not injective')
        assert set(got) == set(want), (b, len(got), len(want))
        rg = new.graph
        if got:
            top = max(float(np.abs(rg.weight).max()), float(np.abs(rg.final[rg.final < INF]).max(initial=0.0)))
        for key, p in got.items():
            tol = (len(p) + 1) * 2.0 ** -24 * top
            assert abs(RC.path_graph_cost(new, p) - want[key]) <= tol, (b, key)
            assert [float(new.lp[j]) for j in p] == [float(old.lp[old_arc[i]]) for i in key]     # the acoustic side
        total += len(got)
        if not want:
            assert new.num_nodes == 0 and new.cost == np.float32(INF)
        else:
            assert abs(float(new.cost) - new.best_path()[1]) <= 1e-4
    assert total > 0
    print('case %d scale %s: %d rescored paths, stats %s' % (k, scale, total, res.stats))


def test_canonical_form():
    for k in range(len(RC.BRUTE)):
        _, lats, lm = RC.brute_case(k)
        res = LatticeBatch(lats).rescore_lm(lm)
        for lat in res.lattices:
            key = lat.time.astype(np.int64) * lat.graph.num_states + lat.state
            assert len(np.unique(key)) == lat.num_nodes
            assert (np.diff(key) > 0).all()                                     # nodes by (time, state)
            akey = lat.src.astype(np.int64) * len(lat.graph.src) + lat.arc
            assert (np.diff(akey) > 0).all()                                    # arcs by (src, arc)
            assert (lat.graph.src[lat.arc] == lat.state[lat.src]).all()
            assert (lat.graph.dst[lat.arc] == lat.state[lat.dst]).all()
        batch = DeviceLatticeBatch.from_lattices(res.lattices, 'cpu')           # validates levels and order
        assert batch.best_paths()[0] == res.best_paths()
        rg = res.lattices[0].graph
        pairs = rg.state_pairs
        assert (np.diff(pairs[:, 0] * lm.num_states() + pairs[:, 1]) > 0).all()
        assert tuple(pairs[rg.start]) == (rg.base.start, lm.start())
        assert (np.diff(rg.src * len(rg.base.src) + rg.arc_base) > 0).all()     # arcs by (source id, base arc)
        assert (rg.ilabel == rg.base.ilabel[rg.arc_base]).all() and (rg.olabel == rg.base.olabel[rg.arc_base]).all()


def test_trivial_lm():
    for k in range(len(RC.BRUTE)):
        _, lats, _ = RC.brute_case(k)
        res = LatticeBatch(lats).rescore_lm(RC.trivial_lm())
        for old, new in zip(lats, res.lattices):
            # the search keeps arcs by its own traceback and beam; everything on a complete path stays
            on_path = sorted({j for p in RC.complete_paths(old) for j in p})
            assert new.num_arcs == len(on_path)
            rg = new.graph
            assert (rg.arc_base[new.arc] == old.arc[on_path]).all()
            assert (new.lp == old.lp[on_path]).all()
            assert (rg.weight[new.arc] == old.w[on_path]).all()
            nodes = sorted({int(old.src[j]) for j in on_path} | {int(old.dst[j]) for j in on_path})
            assert (new.time == old.time[nodes]).all() and (rg.state_pairs[new.state, 0] == old.state[nodes]).all()
        assert res.best_paths() == LatticeBatch(lats).best_paths()
        assert res.stats['max_lm_states'] == 1 and res.stats['dropped_arcs'] == 0


def test_round_trip():
    for k in range(len(RC.BRUTE)):
        _, lats, lm = RC.brute_case(k)
        out = LatticeBatch(lats).rescore_lm(lm, scale=-1.0)
        back = LatticeBatch(out.lattices).rescore_lm(lm, scale=1.0)
        first = LatticeBatch(lats).rescore_lm(lm, scale=0.0)                    # the paths the LM knows, costs unchanged
        for b, (old, new) in enumerate(zip(lats, back.lattices)):
            rg2 = new.graph
            rg1 = rg2.base
            want = {}
            for p in RC.complete_paths(old):
                if lm_cost(lm, old, RC.path_words(old, p)) < INF:
                    want[identity(old)(p)] = RC.path_graph_cost(old, p)
            got = RC.complete_paths(new)
            assert len(got) == len(want)
            top = max([1.0] + [float(np.abs(x.weight).max()) for x in (rg1, rg2) if len(x.weight)])
            for p in got:
                key = tuple((int(new.time[new.src[j]]), int(rg1.state_pairs[rg2.state_pairs[new.state[new.src[j]], 0], 0]),
                             int(rg1.arc_base[rg2.arc_base[new.arc[j]]])) for j in p)
                # two roundings an arc and two for the final cost
                assert abs(RC.path_graph_cost(new, p) - want[key]) <= 2 * (len(p) + 1) * 2.0 ** -24 * top, (b, key)
        # the same words win
        for old, new in zip(first.best_paths(), back.best_paths()):
            assert old[0] == new[0]


def test_shipped_lms():
    """HC o bigram lattices rescored with the shipped trigram; these draws reach 61 LM states on one node"""
    g, lats, tg, lmap = RC.shipped_case()
    blm = BackoffLm.from_fst(tg)
    for lm in (tg, RC.bigram_lm()):                     # both shipped LMs fit the back-off form
        b = BackoffLm.from_fst(lm)
        assert (b.final_star_all < INF).sum() >= 1 and b.max_chain >= 1
    res = LatticeBatch(lats).rescore_lm(blm, lmap)
    print(res.stats)
    assert 1 < res.stats['max_lm_states'] < lattice_lm.DEFAULT_MAX_LM_STATES
    assert res.stats['dropped_arcs'] == 0 and res.stats['redone_on_host'] == []
    got = res.nbest(5)
    rg = res.lattices[0].graph
    top = float(np.abs(rg.weight).max())
    for b, lat in enumerate(lats):
        every = lat.nbest(EVERY)                        # every distinct word sequence of the lattice
        assert len(every) < EVERY
        ranked = []
        for w, c in every:                              # the LM cost hangs on the words alone: the cheapest
            lm_c = sum(RC.score_words(tg, [int(lmap[x]) for x in w]))      # alignment stays the cheapest
            if lm_c < INF:
                ranked.append((c + lm_c, w))
        ranked.sort()
        arcs = lat.num_frames * (g.num_ranks + 1) + 1   # no path has more arcs than the lattice has levels
        tol = (arcs + 1) * 2.0 ** -24 * top
        assert len(got[b]) == min(5, len(ranked)) > 0
        for (w, c), (want_c, want_w) in zip(got[b], ranked):
            print(b, w, c, want_c)
            assert w == want_w and abs(c - want_c) <= tol, (b, w, want_w, c, want_c, tol)


def forward_backward(lat):
    """fp64 forward and backward costs of a lattice at its own scale, and the best total"""
    g = lat.graph
    x = g.weight[lat.arc].astype(np.float64) - lat.acoustic_scale * lat.lp.astype(np.float64)
    end = np.full(lat.num_nodes, INF)
    at_n = lat.time == lat.num_frames
    end[at_n] = g.final[lat.state[at_n]] if lat.reached_final else 0.0
    fwd = np.full(lat.num_nodes, INF)
    fwd[(lat.time == 0) & (lat.state == g.start)] = 0.0
    for lv in lat._levels():
        for j in lv:
            fwd[lat.dst[j]] = min(fwd[lat.dst[j]], fwd[lat.src[j]] + x[j])
    bwd = end.copy()
    for lv in reversed(lat._levels()):
        for j in lv:
            bwd[lat.src[j]] = min(bwd[lat.src[j]], x[j] + bwd[lat.dst[j]])
    return fwd, bwd, x, float((fwd + end).min())


@pytest.mark.parametrize('X', [0.0, 0.75, 2.0])
def test_pruning(X):
    for k in range(len(RC.BRUTE)):
        _, lats, lm = RC.brute_case(k)
        full = LatticeBatch(lats).rescore_lm(lm)
        cut = LatticeBatch(lats).rescore_lm(lm, lattice_beam=X)
        assert cut.lattices[0].graph.num_states <= full.lattices[0].graph.num_states
        for b, (a, c) in enumerate(zip(full.lattices, cut.lattices)):
            if not a.num_nodes:
                assert not c.num_nodes
                continue
            fwd, bwd, x, best = forward_backward(a)
            assert abs(best - float(a.cost)) <= 1e-4 and c.cost == a.cost
            through = fwd[a.src] + x + bwd[a.dst]
            slack = 64 * 2.0 ** -24 * max(1.0, abs(best))          # rounding of the fp32 sums along a path
            ga, gc = a.graph, c.graph
            ident_a = {(int(a.time[a.src[j]]), tuple(ga.state_pairs[a.state[a.src[j]]]), int(ga.arc_base[a.arc[j]])): j
                       for j in range(a.num_arcs)}
            kept = np.zeros(a.num_arcs, bool)
            for j in range(c.num_arcs):
                kept[ident_a[(int(c.time[c.src[j]]), tuple(gc.state_pairs[c.state[c.src[j]]]), int(gc.arc_base[c.arc[j]]))]] = True
            clear_in, clear_out = through <= best + X - slack, through > best + X + slack
            assert kept[clear_in].all(), (b, X)
            if X > 0:                                   # X = 0 also keeps the traceback's arcs, whatever the rounding
                assert not kept[clear_out].any(), (b, X)
            # a best path is kept
            assert c.best_path()[0] == a.best_path()[0] and abs(c.best_path()[1] - a.best_path()[1]) <= 1e-5
            assert np.isfinite(c.alpha).all() and np.isfinite(c.beta).all()


def test_out_of_vocabulary():
    g, lats, lm = RC.brute_case(0)
    blm = BackoffLm.from_fst(lm)
    assert blm.step(0, 3) is None and blm.step(0, 7) is None        # no unigram: nothing matches from the unigram state
    res = LatticeBatch(lats).rescore_lm(lm)
    assert res.stats['dropped_arcs'] > 0
    # a map that knows no word kills every path with a word on it
    none = np.full(RC.N_WORDS + 1, -1)
    none[0] = 0
    dead = LatticeBatch(lats).rescore_lm(lm, label_map=none)
    for old, new in zip(lats, dead.lattices):
        silent = [p for p in RC.complete_paths(old) if not RC.path_words(old, p)
                  and lm_cost(lm, old, []) < INF]
        assert len(RC.complete_paths(new)) == len(silent)
        if not silent:
            assert new.num_nodes == 0 and new.num_arcs == 0 and new.cost == np.float32(INF) and not new.reached_final
    assert any(l.num_nodes == 0 for l in dead.lattices)
    # one utterance dies, the others are what they are without it
    only = np.arange(RC.N_WORDS + 1)
    words = [set(RC.path_words(l, range(l.num_arcs))) for l in lats]
    victim = 1
    for w in words[victim]:
        only[w] = -1
    part = LatticeBatch(lats).rescore_lm(lm, label_map=only, oov_cost=INF)
    alone = [LatticeBatch([l]).rescore_lm(lm, label_map=only).lattices[0] for l in lats]
    for got, want in zip(part.lattices, alone):
        assert got.num_nodes == want.num_nodes and (got.alpha == want.alpha).all() and got.cost == want.cost
        assert got.best_path() == want.best_path()
    # a finite oov cost keeps the arcs at that cost and the LM state where the chain ended
    kept = LatticeBatch(lats).rescore_lm(lm, label_map=none, oov_cost=2.5)
    assert kept.stats['dropped_arcs'] == 0 and kept.stats['max_lm_states'] == 1
    for old, new in zip(lats, kept.lattices):
        rg = new.graph
        paths = RC.complete_paths(new)
        assert len(paths) == len([p for p in RC.complete_paths(old) if lm_cost(lm, old, []) < INF])
        word = rg.olabel != 0
        assert np.allclose(rg.weight[word], rg.base.weight[rg.arc_base[word]] + 2.5, atol=1e-6)
        assert (rg.weight[~word] == rg.base.weight[rg.arc_base[~word]]).all()
        assert (rg.state_pairs[:, 1] == lm.start()).all()


def test_malformed_lms():
    fin = [INF, INF, 0.0]
    two = LmFst(4, 0, [0, 0, 0, 1, 2], [1, 2, 1, 3, 3], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1], [1.0] * 5, fin + [0.0])
    with pytest.raises(ValueError, match='two back-off'):
        BackoffLm.from_fst(two)
    dup = LmFst(3, 0, [0, 0, 1], [1, 2, 2], [1, 1, 2], [1, 1, 2], [1.0] * 3, fin)
    with pytest.raises(ValueError, match='one label'):
        BackoffLm.from_fst(dup)
    cyc = LmFst(3, 0, [0, 1, 0, 1], [1, 0, 2, 2], [0, 0, 1, 1], [0, 0, 1, 1], [1.0] * 4, fin)
    with pytest.raises(ValueError, match='cycle'):
        BackoffLm.from_fst(cyc)
    _, lats, lm = RC.brute_case(0)
    with pytest.raises(ValueError):
        LatticeBatch(lats).rescore_lm(lm, max_lm_states=0)
    with pytest.raises(ValueError):
        LatticeBatch(lats).rescore_lm(lm, scale=float('nan'))


def test_back_off_form():
    rng = np.random.default_rng(4)
    lm = RC.random_backoff_lm(rng)
    blm = BackoffLm.from_fst(lm)
    assert blm.max_chain >= 2                           # two back-off levels (the bound also counts the sink)
    for _ in range(200):
        words = rng.integers(1, RC.N_WORDS + 1, int(rng.integers(0, 5))).tolist()
        q, c, ok = blm.start(), 0.0, True
        for w in words:
            s = blm.step(q, w)
            if s is None:
                ok = False
                break
            q, c = s[0], c + s[1]
        arcs, end = RC.score_words(lm, words)
        if not ok:
            assert arcs == INF
        else:
            assert abs(c - arcs) <= 1e-12 and (blm.final_star(q) == end or abs(blm.final_star(q) - end) <= 1e-12)


def test_switch_and_cpu_batch(monkeypatch):
    _, lats, lm = RC.brute_case(0)
    batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = batch.rescore_lm(lm, lattice_beam=1.0)
    want = LatticeBatch(lats).rescore_lm(lm, lattice_beam=1.0)
    assert res.stats == want.stats
    for x, y in zip(res.lattices(), want.lattices):
        for f in Lattice.FIELDS:
            assert getattr(x, f).tobytes() == getattr(y, f).tobytes(), f
    assert res.best_paths()[0] == want.best_paths()
    # an empty lattice keeps its place
    mixed = [lats[0], _empty(lats[0].graph, 1.0, 4), lats[1]]
    res = LatticeBatch(mixed).rescore_lm(lm)
    assert res.lattices[1].num_nodes == 0 and res.lattices[1].cost == np.float32(INF)
    assert res.best_paths()[2] == LatticeBatch(lats).rescore_lm(lm).best_paths()[1]


def test_abi():
    L = _native.lib()
    assert L.asr_abi_version() == 24
    cap = lattice_lm.DEFAULT_MAX_LM_STATES
    assert cap >= 256 and lattice_lm.DEVICE_MAX_LM_STATES >= cap
    assert L.asr_lattice_lmrescore_supported(0, 0, 0, cap) == 1
    assert L.asr_lattice_lmrescore_supported(1000, 5000, 40, lattice_lm.DEVICE_MAX_LM_STATES) == 1
    assert L.asr_lattice_lmrescore_supported(-1, 0, 0, cap) == 0
    assert L.asr_lattice_lmrescore_supported(0, -1, 0, cap) == 0
    assert L.asr_lattice_lmrescore_supported(0, 0, 0, 0) == 0
    assert L.asr_lattice_lmrescore_supported(0, 0, 0, lattice_lm.DEVICE_MAX_LM_STATES + 1) == 0
    assert L.asr_lattice_lmrescore_supported(2 ** 31, 0, 0, cap) == 0
    assert L.asr_lattice_lmrescore_workspace_bytes(0, cap) == 16
    assert L.asr_lattice_lmrescore_workspace_bytes(10, cap) >= 10 * cap * 4
    assert L.asr_lattice_lmrescore_workspace_bytes(-1, cap) == 0
    assert L.asr_lattice_lmrescore_workspace_bytes(10, 0) == 0
    assert L.asr_lattice_lmrescore_workspace_bytes(10, -3) == 0
