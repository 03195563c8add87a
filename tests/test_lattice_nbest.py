"""LatticeBatch.nbest (att_speech/wfst_lattice.py), the numpy twin of asr_lattice_nbest_f64, on the
CPU: against the best-first search Lattice.nbest and the brute-force enumerator
(tests/wfst_lattice_referee.py) on the toy sweep, on unquantised scores over the shipped bigram LM
graph, against best_paths at n = 1, and the host path of DeviceLatticeBatch.nbest, FSTDecoder, the
tool and the C argument checks on top (no GPU needed).

The one documented difference from Lattice.nbest: sequences that tie at the n-th cost are cut by
(length, hash) here and by the words there, so the cost lists are compared with == and the word
lists through their costs (tests/nbest_cases.py: check_against_host)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import lattice_dp_referee as DR
import nbest_cases as NC
import wfst_lattice_referee as LR
import wfst_referee as R
from grammar_cases import BIGRAM_LM, WSJ_VOCAB
from wfst_cases import INF, TOYS, grid_scores, toy_graph

from att_speech import _native, lattice_dp
from att_speech.lattice_dp import DeviceLatticeBatch, decode_lattice_device
from att_speech.wfst_lattice import NBEST_HASH_MUL, LatticeBatch, decode_lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', sorted(TOYS))
def test_twin_against_the_host_search_on_the_toy_sweep(name):
    cases = identical = 0
    g, lp = NC.toy_inputs(name)
    for _, scale, lb in [c for c in NC.sweep() if c[0] == name]:
        lats, every = NC.toy_lattices(name, scale, lb)
        batch = LatticeBatch(lats)
        for n in NC.sweep_ns(every):
            got = batch.nbest(n)
            assert len(got) == len(lats)
            for b, lat in enumerate(lats):
                NC.check_against_host(got[b], lat, every[b], n, (name, scale, lb, n, b))
                cases += 1
                identical += got[b] == lat.nbest(n)
                if lb == INF:       # the lattice holds every path: the enumerator's sequences and costs
                    _, paths = LR.paths_within(R.graph_args(g), lp[:, b], NC.LENS[b], lb, scale)
                    want = LR.nbest_of(paths, n)
                    assert [c for _, c in got[b]] == [c for _, c in want]
                    assert n < len(every[b]) or got[b] == want
    assert cases == 200                                 # 600 over the three toys, none skipped
    assert identical >= cases // 2                      # ties at the cut are the exception


def test_unquantised_scores_on_the_bigram_graph():
    """fp64 sums of up to 3 * 25 terms below 1e3: 1e-9 is the bound the posteriors are held to"""
    gaps = []
    for lb in NC.UNQUANTISED_BEAMS:
        lats = NC.unquantised_lattices(lb)
        batch = LatticeBatch(lats)
        for n in (5, 20):
            got = batch.nbest(n)
            for b, lat in enumerate(lats):
                want = lat.nbest(n)
                assert [w for w, _ in got[b]] == [w for w, _ in want], (lb, n, b)
                diff = [abs(c - d) for (_, c), (_, d) in zip(got[b], want)]
                print(lb, n, b, len(want), 'max |cost diff|', max(diff))
                assert max(diff) <= 1e-9
                gaps += list(np.diff([c for _, c in want]))
    assert len(gaps) > 100 and min(gaps) > 1e-6         # the order is decided by the costs, not by ties


@pytest.mark.parametrize('name', sorted(TOYS))
def test_nbest_1_is_the_best_path(name):
    for lb in (0.0, 2.0, INF):
        lats, every = NC.toy_lattices(name, 1.0, lb)
        batch = LatticeBatch(lats)
        for sc, lm in ((None, 1.0), (0.5, 1.0), (0.5, 2.0)):
            best = batch.best_paths(sc, lm)
            got = batch.nbest(1, sc, lm)
            for b, lat in enumerate(lats):
                assert len(got[b]) == 1 and got[b][0][1] == best[b][1], (name, lb, sc, lm, b)
                costs = [c for _, c in lat.nbest(2, sc, lm)]
                if len(costs) < 2 or costs[0] < costs[1]:
                    assert got[b][0][0] == best[b][0]


def test_scale_pairs_and_the_nan_corner():
    for name in sorted(TOYS):
        lats, _ = NC.toy_lattices(name, 1.0, 2.0)
        batch = LatticeBatch(lats)
        every = [lat.nbest(10 ** 6, 0.5, 2.0) for lat in lats]
        for n in (1, 3, 10, 1000):
            got = batch.nbest(n, 0.5, 2.0)
            for b, lat in enumerate(lats):
                want = lat.nbest(n, 0.5, 2.0)
                assert [c for _, c in got[b]] == [c for _, c in want]
                assert n < len(every[b]) or got[b] == want
        # lm_scale = 0: e(v) = 0 * inf = NaN where the final cost is +inf, and NaN < inf is false: such a
        # node ends no path but passes paths on.  (Lattice.nbest agrees on the ends, but its cost-to-go
        # is a NaN-propagating minimum, so it also loses every path THROUGH such a node; the enumerator
        # of tests/lattice_dp_referee.py scores the paths one by one and is the referee here.)
        got, full = batch.nbest(5, 1.0, 0.0), batch.nbest(10 ** 4, 1.0, 0.0)
        for b, lat in enumerate(lats):
            paths = [(p['cost'], None, p['words']) for p in DR.scored_paths(lat, 1.0, 0.0)]
            assert [c for _, c in got[b]] == [c for _, c in LR.nbest_of(paths, 5)], (name, b)
            assert full[b] == LR.nbest_of(paths, 10 ** 4), (name, b)
            with np.errstate(invalid='ignore'):
                assert {tuple(w) for w, _ in lat.nbest(10 ** 6, 1.0, 0.0)} <= {tuple(p[2]) for p in paths}
        assert all(row for row in got)


def test_empty_partial_and_wordless_lattices():
    g = toy_graph('c')                                  # its final state is at least three frames away
    lens = [1, 5, 2]
    lp = torch.from_numpy(grid_scores(np.random.default_rng(4), 5, 3, 3, lens, low=-4.0))
    gone = decode_lattice(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=False)[0]
    part = decode_lattice(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=True)[0]
    mixed = [gone[0], gone[1], part[2]]
    assert [l.num_nodes > 0 for l in mixed] == [False, True, True] and not part[2].reached_final
    got = LatticeBatch(mixed).nbest(4)
    assert got[0] == [] and got[1] and got[2]
    for b in (1, 2):
        assert [c for _, c in got[b]] == [c for _, c in mixed[b].nbest(4)]
    assert LatticeBatch([]).nbest(3) == [] and LatticeBatch(mixed).nbest(0) == [[], [], []]
    assert LatticeBatch([gone[0], gone[2]]).nbest(3) == [[], []]
    # every output label 0: all paths are one sequence, the empty one, at the best path's cost
    lat = NC.toy_lattices('a', 1.0, INF)[0][0]
    silent = NC.without_words(lat)
    assert LatticeBatch([silent]).nbest(7)[0] == [([], silent.best_path()[1])] == silent.nbest(7)


def test_fan_lattice_ties_and_duplicates():
    """thousands of arcs at one node, costs that tie in hundreds, labels that repeat"""
    lat = NC.fan_lattice()
    out = np.bincount(lat.src, minlength=lat.num_nodes)
    into = np.bincount(lat.dst, minlength=lat.num_nodes)
    assert out.max() >= 3000 and into.max() >= 3000
    batch = LatticeBatch([lat])
    for n in (10, 64):
        got = batch.nbest(n)[0]
        want = lat.nbest(n)
        assert len(got) == n and [c for _, c in got] == [c for _, c in want]
        assert len({tuple(w) for w, _ in got}) == n
    assert len({c for _, c in got}) < n // 2            # ties indeed


def test_the_hash_is_the_documented_one():
    """H(o, h) = h * 0x9E3779B97F4A7C15 + o + 1 mod 2^64, the empty suffix 0: two sequences of one
    length are told apart by it alone"""
    assert NBEST_HASH_MUL == 0x9E3779B97F4A7C15

    def h(words):
        v = 0
        for o in reversed(words):
            v = (v * NBEST_HASH_MUL + o + 1) % 2 ** 64
        return v
    assert h([]) == 0 and h([5]) == 6 and h([1, 2]) != h([2, 1]) and h([0, 0]) != h([0])


@pytest.mark.parametrize('name', sorted(TOYS))
def test_device_batch_host_path_and_sentences(name, monkeypatch):
    lats, every = NC.toy_lattices(name, 1.0, 2.0)
    batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
    host = LatticeBatch(lats)
    for n in (1, 3, lattice_dp.NBEST_DEVICE_MAX + 1):
        assert batch.nbest(n) == host.nbest(n)
        assert batch.sentences(n) == [[w for w, _ in row] for row in host.nbest(n)]
    assert batch.nbest(3, 0.5, 2.0) == host.nbest(3, 0.5, 2.0)
    assert batch.nbest(3, acoustic_scale=0.5, workspace_bytes=1 << 20) == host.nbest(3, 0.5)
    monkeypatch.setenv('ASR_LATTICE_NBEST_NATIVE', '0')
    assert batch.nbest(3) == host.nbest(3)
    g, lp = NC.toy_inputs(name)
    made, redone = decode_lattice_device(torch.from_numpy(lp), NC.LENS, g, beam=INF, lattice_beam=2.0)
    assert redone == [] and made.nbest(4) == host.nbest(4)
    assert lattice_dp.NBEST_DEVICE_MAX >= 64


def test_fst_decoder_device_nbest_on_the_shipped_bigram_lm():
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    kw = dict(normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab, decode_beam=16.0,
              decode_lattice_beam=4.0, decode_nbest=5)
    torch.manual_seed(0)
    plain = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), **kw)
    dev = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), decode_nbest_device=True, **kw)
    both = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), decode_nbest_device=True,
                      decode_confidence=True, **kw)
    assert plain.decode_nbest_device is False and dev.decode_nbest_device is True
    dev.load_state_dict(plain.state_dict())
    both.load_state_dict(plain.state_dict())
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    with torch.no_grad():
        want = plain.decode(enc, elens)
        got = dev.decode(enc, elens)
        conf = both.decode(enc, elens)
    assert got['decoded'] == want['decoded'] and 'word_confidence' not in got
    assert conf['nbest'] == got['nbest'] and len(conf['word_confidence']) == B
    for b in range(B):
        assert [c for _, c in got['nbest'][b]] == pytest.approx([c for _, c in want['nbest'][b]], abs=1e-9)
        assert got['nbest'][b][0][0] == want['nbest'][b][0][0] == want['decoded'][b]
    assert max(len(nb) for nb in got['nbest']) > 1


def test_tool_device_nbest_flag(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import decode_graph as tool
    finally:
        sys.path.pop(0)
    g, lp = NC.toy_inputs('a')
    utts = [('utt%d' % b, lp[:n, b]) for b, n in enumerate(NC.LENS)]
    plain, flagged = tmp_path / 'plain.txt', tmp_path / 'device.txt'
    tool.write_nbest(g, utts, str(plain), beam=INF, lattice_beam=2.0, nbest=3)
    tool.write_nbest(g, utts, str(flagged), beam=INF, lattice_beam=2.0, nbest=3, batch=3, device_nbest=True)
    lats, _ = decode_lattice(torch.from_numpy(np.nan_to_num(lp)), NC.LENS, g, beam=INF, lattice_beam=2.0)
    want = []
    for b, row in enumerate(LatticeBatch(lats).nbest(3)):
        for k, (words, cost) in enumerate(row):
            want.append(' '.join(['utt%d-%d' % (b, k + 1), '%.6f' % cost] + [str(w) for w in words]))
    got = flagged.read_text().splitlines()
    assert got == want and len(got) > 4
    # the same format, the same costs line for line as without the flag
    assert [l.split()[:2] for l in got] == [l.split()[:2] for l in plain.read_text().splitlines()]
    # the command line: the flag reaches write_nbest, and needs --lattice-beam
    seen = {}
    monkeypatch.setattr(tool, 'write_nbest', lambda *a, **k: seen.update(k))
    from att_speech.ctc_forward import KaldiFloatMatrixWriter
    ark, fst = tmp_path / 'lp.ark', tmp_path / 'g.txt'
    with KaldiFloatMatrixWriter(str(ark)) as writer:
        for key, m in utts:
            writer[key] = m
    t = TOYS['a']
    with open(str(fst), 'w') as f:
        for s, il, ol, w, d in t['arcs']:
            f.write('%d %d %d %d %g\n' % (s, d, il, ol, w))
        for s, w in t['final'].items():
            f.write('%d %g\n' % (s, w))
    tool.main([str(ark), str(fst), '--lattice-beam', '2', '--nbest', '3', '--device-nbest', '--device', 'cpu'])
    assert seen['device_nbest'] is True and seen['nbest'] == 3
    tool.main([str(ark), str(fst), '--lattice-beam', '2', '--nbest', '3', '--device', 'cpu'])
    assert seen['device_nbest'] is False
    with pytest.raises(SystemExit):
        tool.main([str(ark), str(fst), '--device-nbest'])


def test_argument_checks_need_no_gpu():
    """n < 1, null pointers, offsets that decrease, a workspace too small: the status comes back
    before anything is launched (no GPU here)"""
    L = _native.lib()
    assert L.asr_abi_version() == 24
    cap = lattice_dp.NBEST_DEVICE_MAX
    assert L.asr_lattice_nbest_supported(10, 20, 5, 1) == 1 and L.asr_lattice_nbest_supported(10, 20, 5, cap) == 1
    assert L.asr_lattice_nbest_supported(10, 20, 5, cap + 1) == 0 and L.asr_lattice_nbest_supported(10, 20, 5, 0) == 0
    assert L.asr_lattice_nbest_supported(2 ** 31, 20, 5, 4) == 0
    assert L.asr_lattice_nbest_workspace_bytes(100, 10) >= 100 * (28 * 10 + 4)
    assert L.asr_lattice_nbest_workspace_bytes(100, 10) <= 100 * (28 * 10 + 4) + 128
    assert L.asr_lattice_nbest_workspace_bytes(100, 0) == 0 and L.asr_lattice_nbest_workspace_bytes(-1, 4) == 0
    assert L.asr_lattice_nbest_workspace_bytes(100, cap + 1) == 0

    def off(*v):
        a = np.array(v, np.int64)
        return a, a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(64)      # never dereferenced: every case below fails a check on the host

    def call(B, b0, nb, n, N, A, Lv, hn, ha, hl, dev=fake, out=fake, start=0, threads=0, ws=fake, ws_bytes=1 << 20):
        return L.asr_lattice_nbest_f64(B, b0, nb, n, N, A, Lv, hn, ha, hl, *[dev] * 18, 1.0, 1.0, 7, 16, dev, dev,
                                       dev, start, threads, out, out, out, out, out, ws, ws_bytes, None)
    keep = [off(0, 4, 9), off(0, 6, 12), off(0, 3, 6)]
    (_, hn), (_, ha), (_, hl) = keep
    E = _native.ASR_EINVAL
    assert call(2, 0, 2, 0, 9, 12, 6, hn, ha, hl) == E                          # n < 1
    assert call(2, 0, 2, -3, 9, 12, 6, hn, ha, hl) == E
    assert call(2, 0, 2, cap + 1, 9, 12, 6, hn, ha, hl) == _native.ASR_EUNSUPPORTED
    assert call(2, 0, 2, 4, 9, 12, 6, hn, ha, hl, ws_bytes=9 * (28 * 4 + 4)) == E       # workspace too small
    assert call(2, 0, 2, 4, 9, 12, 6, hn, ha, hl, ws=None) == E
    assert call(2, 0, 2, 4, 9, 12, 6, hn, ha, hl, dev=None) == E                # null device pointers
    assert call(2, 0, 2, 4, 9, 12, 6, hn, ha, hl, out=None) == E                # null outputs
    assert call(2, 0, 2, 4, 9, 12, 6, None, ha, hl) == E                        # no host offsets
    assert call(2, 0, 2, 4, 10, 12, 6, hn, ha, hl) == E                         # offsets end short of N
    assert call(2, 1, 2, 4, 9, 12, 6, hn, ha, hl) == E                          # utterances beyond B
    assert call(2, 0, 2, 4, 9, 12, 6, hn, ha, hl, threads=96) == E
    assert call(2, 0, 2, 4, 9, 12, 6, hn, ha, hl, start=7) == E                 # start outside the graph
    down = off(0, 6, 4, 9)
    flat = [off(0, 4, 8, 12), off(0, 2, 4, 6)]
    assert call(3, 0, 3, 4, 9, 12, 6, down[1], flat[0][1], flat[1][1]) == E     # offsets that decrease
    assert call(2, 0, 2, 4, 2 ** 31, 12, 6, hn, ha, hl) == _native.ASR_EUNSUPPORTED
    assert call(2, 0, 0, 4, 9, 12, 6, hn, ha, hl) == _native.ASR_OK             # nothing to do


def test_the_entry_points_are_declared_and_exported():
    names = ('asr_lattice_nbest_supported', 'asr_lattice_nbest_workspace_bytes', 'asr_lattice_nbest_f64')
    handle = ctypes.CDLL(_native.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'asr_amd.h')).read()
    for name in names:
        assert hasattr(handle, name) and name in _native._SIGNATURES and name + '(' in header
    assert '#define ASR_LATTICE_NBEST_MAX %d' % lattice_dp.NBEST_DEVICE_MAX in header
