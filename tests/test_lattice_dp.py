"""att_speech.lattice_dp and the posteriors of att_speech.wfst_lattice on the CPU: the numpy
log-semiring pass against direct summation over every enumerated path
(tests/lattice_dp_referee.py), its invariants, the host path of DeviceLatticeBatch, the argument
checks of the new C entry points (no GPU needed), and the tool and decoder on top.

Inputs: the toys of tests/wfst_cases.py on the 2^-8 grid; frames beyond an utterance's length NaN.

lm_scale = 0 is a posterior case only: LatticeBatch.best_paths multiplies the +inf of the nodes
that end no path by lm_scale, so 0 * inf = NaN leaves every utterance without a best path there
(the device sweep reproduces that, tests/test_lattice_dp_gpu.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import lattice_dp_referee as DR
from grammar_cases import BIGRAM_LM, WSJ_VOCAB
from wfst_cases import INF, TOYS, grid_scores, toy_graph

from att_speech import _native
from att_speech.lattice_dp import DeviceLatticeBatch, decode_lattice_device
from att_speech.wfst_lattice import Lattice, LatticeBatch, decode_lattice

LENS = [5, 1, 3, 5]
LATTICE_BEAMS = (0.0, 2.0, INF)
PAIRS = ((1.0, 1.0), (0.5, 1.0), (1.0, 0.0))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9          # as on the device (tests/test_lattice_dp_gpu.py); the host is far inside it here

_CACHE = {}


def toy_lattices(name, lb):
    if (name, lb) not in _CACHE:
        g = toy_graph(name)
        lp = grid_scores(np.random.default_rng(len(name) + 3), 5, 4, 3, LENS, low=-4.0)
        _CACHE[name, lb] = decode_lattice(torch.from_numpy(lp), LENS, g, beam=INF, lattice_beam=lb)[0]
    return _CACHE[name, lb]


def assert_log_close(got, want, what):
    """log values: -inf in the same places; 1e-9 above -30, below that 1e-12 on the linear value"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    big = want > -30.0
    assert (np.abs(got[big] - want[big]) <= TOL).all(), (what, got[big], want[big])
    assert (np.abs(np.exp(got[~big]) - np.exp(want[~big])) <= 1e-12).all(), what
    assert ((got == -INF) == (want == -INF)).all(), what


@pytest.mark.parametrize('name', sorted(TOYS))
def test_host_posteriors_against_the_enumerator(name):
    for lb in LATTICE_BEAMS:
        lats = toy_lattices(name, lb)
        batch = LatticeBatch(lats)
        for sc, lm in PAIRS:
            post = batch.posteriors(sc, lm)
            assert post.log_z.dtype == np.float64 and post.arc_log_post.dtype == np.float64
            assert len(post.arc_log_post) == sum(l.num_arcs for l in lats)
            assert len(post.node_log_post) == sum(l.num_nodes for l in lats)
            a0 = n0 = 0
            for b, lat in enumerate(lats):
                log_z, arcs, nodes = DR.posteriors(lat, sc, lm)
                what = (name, lb, sc, lm, b)
                assert_log_close([post.log_z[b]], [log_z], what)
                assert_log_close(post.arc_log_post[a0:a0 + lat.num_arcs], arcs, what)
                assert_log_close(post.node_log_post[n0:n0 + lat.num_nodes], nodes, what)
                one = lat.posteriors(sc, lm)            # Lattice.posteriors: the batch of one
                assert_log_close(one.arc_log_post, arcs, what)
                a0, n0 = a0 + lat.num_arcs, n0 + lat.num_nodes


@pytest.mark.parametrize('name', sorted(TOYS))
def test_posterior_invariants(name):
    for lb in LATTICE_BEAMS:
        lats = toy_lattices(name, lb)
        post = LatticeBatch(lats).posteriors()
        p = np.exp(post.arc_log_post)
        a0 = 0
        for b, lat in enumerate(lats):
            mine = p[a0:a0 + lat.num_arcs]
            a0 += lat.num_arcs
            emitting = lat.ilabel > 0
            for k in range(1, lat.num_frames + 1):      # every path crosses into time k exactly once
                assert abs(mine[emitting & (lat.time[lat.dst] == k)].sum() - 1.0) < 1e-12, (name, lb, b, k)
            start = np.nonzero((lat.time == 0) & (lat.state == lat.graph.start))[0][0]
            assert abs(mine[lat.src == start].sum() - 1.0) < 1e-12
            if len(DR.complete_paths(lat)) == 1:
                assert (np.abs(mine - 1.0) < 1e-12).all()
        frames = post.frame_posteriors(num_classes=3)     # default: the classes the graph reads
        assert frames.shape == (5, 4, 3) and frames.dtype == torch.float32
        for b, n in enumerate(LENS):
            assert (frames[:n, b].sum(-1) - 1.0).abs().max() < 1e-5
            assert (frames[n:, b] == 0).all()
    single = [len(DR.complete_paths(lat)) for lat in toy_lattices('c', 0.0)]
    assert single == [1, 1, 1, 1]                       # the single-path case above did run


@pytest.mark.parametrize('name', sorted(TOYS))
def test_host_best_paths_and_round_trip(name):
    """DeviceLatticeBatch on CPU tensors: the host path.  A sequence of scales equals the per-scale
    calls, which equal the enumerator; from_lattices(...).lattices() gives every field back."""
    for lb in LATTICE_BEAMS:
        lats = toy_lattices(name, lb)
        batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
        scales = [1.0, None, 0.5, 0.1]
        lms = [1.0, 1.0, 1.0, 2.0]
        got = batch.best_paths(scales, lms)
        host = LatticeBatch(lats)
        assert got == [host.best_paths(sc, lm) for sc, lm in zip(scales, lms)]
        assert batch.best_paths(0.5) == [host.best_paths(0.5)]
        assert batch.best_paths([1.0, 0.5], 2.0) == [host.best_paths(1.0, 2.0), host.best_paths(0.5, 2.0)]
        for k, (sc, lm) in enumerate(zip(scales, lms)):
            for b, lat in enumerate(lats):
                assert got[k][b] == DR.best_path(lat, sc, lm), (name, lb, sc, lm, b)
        back = batch.lattices()
        assert len(back) == len(lats)
        for a, b in zip(back, lats):
            assert isinstance(a, Lattice) and a.graph is b.graph
            assert (a.acoustic_scale, a.num_frames, a.reached_final) == (b.acoustic_scale, b.num_frames,
                                                                         b.reached_final)
            assert a.cost == b.cost and a.cost.dtype == b.cost.dtype
            for f in Lattice.FIELDS:
                x, y = getattr(a, f), getattr(b, f)
                assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), f
    with pytest.raises(ValueError):
        batch.best_paths([1.0, 0.5], [1.0, 1.0, 1.0])


def test_decode_lattice_device_on_the_cpu_and_empty_lattices():
    g = toy_graph('c')                                  # its final state is at least three frames away
    lens = [1, 5, 2]
    lp = grid_scores(np.random.default_rng(4), 5, 3, 3, lens, low=-4.0)
    want, _ = decode_lattice(torch.from_numpy(lp), lens, g, beam=INF, lattice_beam=2.0, allow_partial=False)
    batch, redone = decode_lattice_device(torch.from_numpy(lp), lens, g, beam=INF, lattice_beam=2.0,
                                          allow_partial=False)
    assert redone == [] and batch.num_utterances == 3
    assert [l.num_nodes > 0 for l in want] == [False, True, False]
    got = batch.lattices()
    for a, b in zip(got, want):
        assert a.cost == b.cost and a.num_frames == b.num_frames and a.reached_final == b.reached_final
        for f in Lattice.FIELDS:
            assert (getattr(a, f) == getattr(b, f)).all()
    none = ([], INF, INF, INF)
    best = batch.best_paths([1.0, 0.5])
    assert best[0][0] == none and best[0][2] == none and best[1][0] == none and best[0][1] != none
    post = batch.posteriors()
    assert post.log_z[0] == -INF and post.log_z[2] == -INF and np.isfinite(post.log_z[1])
    assert post.word_posteriors()[0] == [] and post.frame_posteriors()[:, 0].abs().sum() == 0


def test_word_posteriors_against_a_hand_count():
    lat = toy_lattices('a', INF)[0]
    post = lat.posteriors()
    words, _, _, _ = lat.best_path()
    paths = DR.scored_paths(lat)
    log_z = DR.posteriors(lat)[0]
    best = min(paths, key=lambda p: p['cost'])
    assert best['words'] == words and len(words) >= 2
    on_path = [j for j in best['arcs'] if lat.olabel[j] != 0]
    for window in (0, 1):
        got = post.word_posteriors(window=window)
        assert len(got) == 1 and [w for w, _, _ in got[0]] == words
        for (word, frame, p), j in zip(got[0], on_path):
            assert word == lat.olabel[j] and frame == lat.time[lat.dst[j]]
            # by hand: every (path, arc) pair whose arc carries the word and ends within the window
            mass = 0.0
            for path in paths:
                hits = sum(1 for a in path['arcs'] if lat.olabel[a] == word
                           and abs(int(lat.time[lat.dst[a]]) - frame) <= window)
                mass += hits * np.exp(-path['cost'] - log_z)
            assert abs(p - min(1.0, mass)) < 1e-12, (window, word, frame, p, mass)
            assert 0.0 < p <= 1.0
    assert any(p < 0.999 for _, _, p in post.word_posteriors(0)[0])


def test_malformed_batches_are_refused():
    lats = toy_lattices('a', 2.0)

    def broken(field, index, value):
        lat = lats[0]
        arrays = {f: getattr(lat, f).copy() for f in Lattice.FIELDS}
        arrays[field][index] = value
        bad = Lattice(lat.graph, lat.acoustic_scale, lat.num_frames, lat.cost, lat.reached_final,
                      *[arrays[f] for f in Lattice.FIELDS])
        return [bad] + list(lats[1:])
    n = lats[0].num_nodes
    for field, index, value in (('src', 3, n), ('dst', 3, -1), ('dst', 0, n + 2), ('arc', 1, 10 ** 6),
                                ('state', 2, 99)):
        with pytest.raises(ValueError):
            DeviceLatticeBatch.from_lattices(broken(field, index, value), 'cpu')
    j = int(np.nonzero(lats[0].src != lats[0].dst)[0][0])
    with pytest.raises(ValueError, match='level'):      # an arc turned round: its level falls
        lat = lats[0]
        arrays = {f: getattr(lat, f).copy() for f in Lattice.FIELDS}
        arrays['src'][j], arrays['dst'][j] = lat.dst[j], lat.src[j]
        DeviceLatticeBatch.from_lattices([Lattice(lat.graph, 1.0, lat.num_frames, lat.cost, True,
                                                  *[arrays[f] for f in Lattice.FIELDS])], 'cpu')


def test_argument_checks_need_no_gpu():
    """Offsets that do not increase, counts that disagree, null pointers, a workspace too small:
    the status comes back before anything is launched (no GPU here)."""
    L = _native.lib()
    assert L.asr_abi_version() == 24
    assert L.asr_lattice_bestpath_supported(10, 20, 5) == 1 and L.asr_lattice_bestpath_supported(2 ** 31, 1, 1) == 0
    assert L.asr_lattice_posterior_supported(10, 20, 5) == 1 and L.asr_lattice_posterior_supported(1, -1, 1) == 0
    assert L.asr_lattice_bestpath_workspace_bytes(100, 3) >= 12 * 300
    assert L.asr_lattice_bestpath_workspace_bytes(100, 0) == 0
    assert L.asr_lattice_posterior_workspace_bytes(100) >= 1600

    def off(*v):
        a = np.array(v, np.int64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(64)      # never dereferenced: every case below fails a check on the host

    def best(B, b0, nb, P, N, A, Lv, hn, ha, hl, dev=fake, start=0, threads=0, ws=fake, ws_bytes=1 << 20, S=7):
        return L.asr_lattice_bestpath_f64(B, b0, nb, P, N, A, Lv, hn, ha, hl, *[dev] * 20, S, 16, dev, dev, dev,
                                          start, threads, dev, dev, dev, dev, ws, ws_bytes, None)

    def post(B, b0, nb, N, A, Lv, hn, ha, hl, dev=fake, ws=fake, ws_bytes=1 << 20):
        return L.asr_lattice_posterior_f64(B, b0, nb, N, A, Lv, hn, ha, hl, *[dev] * 18, 1.0, 1.0, 7, 16, dev, dev,
                                           dev, 0, 0, dev, dev, dev, dev, ws, ws_bytes, None)
    keep = [off(0, 4, 9), off(0, 6, 12), off(0, 3, 6)]
    (_, hn), (_, ha), (_, hl) = keep
    E = _native.ASR_EINVAL
    assert best(2, 0, 2, 1, 9, 12, 6, hn, ha, hl, ws_bytes=8) == E              # workspace too small
    assert post(2, 0, 2, 9, 12, 6, hn, ha, hl, ws_bytes=8) == E
    assert best(2, 0, 2, 1, 9, 12, 6, hn, ha, hl, ws=None) == E
    assert best(2, 0, 2, 1, 9, 12, 6, hn, ha, hl, dev=None) == E                # null device pointers
    assert post(2, 0, 2, 9, 12, 6, hn, ha, hl, dev=None) == E
    assert best(2, 0, 2, 1, 9, 12, 6, None, ha, hl) == E                        # no host offsets
    assert best(2, 0, 2, 1, 10, 12, 6, hn, ha, hl) == E                         # offsets end short of N
    assert best(2, 1, 2, 1, 9, 12, 6, hn, ha, hl) == E                          # utterances beyond B
    assert best(2, 0, 2, -1, 9, 12, 6, hn, ha, hl) == E
    assert best(2, 0, 2, 1, 9, 12, 6, hn, ha, hl, threads=96) == E
    assert best(2, 0, 2, 1, 9, 12, 6, hn, ha, hl, start=7) == E                 # start outside the graph
    down = off(0, 6, 4, 9)
    flat = [off(0, 4, 8, 12), off(0, 2, 4, 6)]
    assert best(3, 0, 3, 1, 9, 12, 6, down[1], flat[0][1], flat[1][1]) == E     # offsets that decrease
    assert post(3, 0, 3, 9, 12, 6, down[1], flat[0][1], flat[1][1]) == E
    few = off(0, 1, 6)
    assert best(2, 0, 2, 1, 9, 12, 6, hn, ha, few[1]) == E                      # arcs but one level
    many = off(0, 5, 6)
    assert post(2, 0, 2, 9, 12, 6, hn, ha, many[1]) == E                        # more levels than nodes
    assert best(2, 0, 2, 1, 2 ** 31, 12, 6, hn, ha, hl) == _native.ASR_EUNSUPPORTED
    assert best(2, 0, 0, 1, 9, 12, 6, hn, ha, hl) == _native.ASR_OK             # nothing to do
    assert post(2, 1, 0, 9, 12, 6, hn, ha, hl) == _native.ASR_OK


def test_tool_post_mode(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import decode_graph as tool
    finally:
        sys.path.pop(0)
    g = toy_graph('a')
    lp = grid_scores(np.random.default_rng(4), 5, 4, 3, LENS, low=-4.0)
    utts = [('utt%d' % b, lp[:n, b]) for b, n in enumerate(LENS)]
    out = tmp_path / 'post.npz'
    tool.write_post(g, utts, str(out), beam=INF, lattice_beam=2.0, batch=3)        # two batches
    got = np.load(str(out))
    assert sorted(got.files) == ['utt0', 'utt1', 'utt2', 'utt3']
    lats, _ = decode_lattice(torch.from_numpy(np.nan_to_num(lp)), LENS, g, beam=INF, lattice_beam=2.0)
    for b, n in enumerate(LENS):
        m = got['utt%d' % b]
        assert m.shape == (n, 3) and m.dtype == np.float32
        assert np.abs(m.sum(-1) - 1.0).max() < 1e-5
        want = lats[b].posteriors().frame_posteriors(n, 3)[:, 0].numpy()
        assert np.abs(m - want).max() < 1e-6
    # the sweep goes through the same batch: the file equals the per-scale host calls
    sweep = tmp_path / 'sweep.txt'
    tool.write_sweep(g, utts, str(sweep), beam=INF, lattice_beam=2.0, scales=[0.5, 1.0], batch=3)
    want = []
    for scale in (0.5, 1.0):
        for b, (words, cost, _, _) in enumerate(LatticeBatch(lats).best_paths(scale)):
            want.append(' '.join(['%g' % scale, 'utt%d' % b, '%.6f' % cost] + [str(w) for w in words]))
    assert sweep.read_text().splitlines() == want


def test_fst_decoder_word_confidence_on_the_shipped_bigram_lm():
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    kw = dict(normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab, decode_beam=16.0,
              decode_lattice_beam=4.0, decode_nbest=5)
    torch.manual_seed(0)
    plain = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), **kw)
    conf = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), decode_confidence=True, **kw)
    assert plain.decode_confidence is False
    conf.load_state_dict(plain.state_dict())
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    with torch.no_grad():
        want = plain.decode(enc, elens)
        got = conf.decode(enc, elens)
    assert 'word_confidence' not in want
    assert got['decoded'] == want['decoded'] and got['nbest'] == want['nbest']
    for b in range(B):
        c = got['word_confidence'][b]
        assert len(c) == len(got['nbest'][b][0][0]) and all(0.0 < p <= 1.0 for p in c)
    assert any(p < 0.999 for c in got['word_confidence'] for p in c)
    with pytest.raises(ValueError):
        FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), normalize_by_dim=None,
                   denominator_red='logsumexp', vocabulary=vocab, decode_beam=16.0, decode_confidence=True)
