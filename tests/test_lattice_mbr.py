"""LatticeBatch.mbr (att_speech/wfst_lattice.py), the numpy twin of asr_lattice_mbr_f64, against the
referee of tests/mbr_referee.py.  The twin is compared at evaluation only (max_iterations=0 with given
hypotheses): the risk is continuous in the inputs and is held to 1e-6, a decade under delta = 1e-5,
the smallest quantity that decides anything, and decades over the fixed-point bound (levels x in-degree
x 2^-41).  The discrete outputs are not compared across arithmetics."""
import numpy as np
import pytest

import mbr_cases as MC
import mbr_referee as MR
import nbest_cases as NC

from att_speech.wfst_lattice import INF, MBR_MASS, MBR_NONE, LatticeBatch, MBRResult, _empty

RISK_TOL = 1e-6

_REF = {}


def referee(name, lat):
    """per probe hypothesis (hyp, risk, gamma) of the scalar referee, computed once"""
    if name not in _REF:
        _REF[name] = [(h,) + MR.evaluate(lat, h) for h in MC.probe_hypotheses(lat)]
    return _REF[name]


def check_sausage(res):
    for row in res.sausage:
        assert abs(sum(g for _, g in row) - 1.0) <= 1e-9, row
        assert row == sorted(row, key=lambda e: (-e[1], e[0]))


def check_slot_masses(lat, hyp):
    """sum over w of gamma(q, w) = 1 for EVERY slot q = 1 .. S, on the raw (slot, word) table: the gap
    slots that hold word 0 alone, which the sausage leaves out, are where mass lost in the case-3 chain
    or at the start node would show"""
    hb = LatticeBatch([lat])
    arc, end = hb.conditionals()
    first = np.array([int(np.nonzero(hb.start)[0][0])])
    _, tables = hb._mbr_evaluate([list(hyp)], np.array([True]), arc, end, first)
    S = 2 * len(hyp) + 1
    mass = [0] * (S + 1)
    for (q, _), (g, _) in tables[0].items():
        assert 1 <= q <= S and g > 0
        mass[q] += g
    for q in range(1, S + 1):
        assert abs(mass[q] / MBR_MASS - 1.0) <= 1e-9, (q, mass[q] / MBR_MASS)


@pytest.mark.parametrize('name,lat', MC.all_lattices(), ids=[n for n, _ in MC.all_lattices()])
def test_risk_against_the_scalar_referee(name, lat):
    if not lat.num_nodes:
        assert lat.mbr() == MBR_NONE
        return
    for hyp, want, gamma in referee(name, lat):
        got = lat.mbr(max_iterations=0, hypothesis=hyp)
        print(name, hyp, got.risk, want, abs(got.risk - want))
        assert got.words == list(hyp) and got.iterations == 1
        assert abs(got.risk - want) <= RISK_TOL, (name, hyp, got.risk, want)
        check_sausage(got)
        check_slot_masses(lat, hyp)
        for k, w in enumerate(hyp):                 # the confidences are continuous where no case ties
            assert 0.0 <= got.confidence[k] <= 1.0 + 1e-9


@pytest.mark.parametrize('name,lat', MC.enumerable(), ids=[n for n, _ in MC.enumerable()])
def test_risk_bounds_the_expected_edit_distance(name, lat):
    """a minimum of expectations bounds the expectation of minima from above"""
    if not lat.num_nodes:
        return
    for hyp in MC.probe_hypotheses(lat):
        E = MR.expected_edit_distance(lat, hyp)
        risk = lat.mbr(max_iterations=0, hypothesis=hyp).risk
        print(name, hyp, risk, E)
        assert risk >= E - RISK_TOL, (name, hyp, risk, E)
        if name in ('tree', 'single', 'silent'):    # one in-arc per node: the recursion is exact
            # E <= risk in exact arithmetic, with equality where no substitution or insertion is paid (the
            # wordless tree, the single path, the empty sentence).  There the 2^-40 fixed point lands on
            # either side of E: FIXED is its bound, (levels x in-degree) 2^-41, with the tree's 5 levels
            # and E's 36 stop arcs as the in-degree; the referee's fsum adds less than 1e-15
            FIXED = 5 * 36 * 2.0 ** -41
            assert E - FIXED <= risk <= E * (1 + MR.DELTA) + RISK_TOL, (name, hyp, risk, E)


def test_single_path():
    lat = MC.single_path()
    res = lat.mbr()
    assert res.words == [3, 4, 4, 2] and res.confidence == [1.0] * 4 and res.risk == 0.0 and res.iterations == 1
    assert res.frames == [1, 3, 4, 5]
    assert res.sausage == [[(3, 1.0)], [(4, 1.0)], [(4, 1.0)], [(2, 1.0)]]
    far = lat.mbr(hypothesis=[9, 9])                # a foreign start: the updates lower the risk
    assert far.iterations >= 2 and far.risk < lat.mbr(max_iterations=0, hypothesis=[9, 9]).risk
    assert far.risk == lat.mbr(max_iterations=0, hypothesis=far.words).risk


def test_mbr_lowers_the_risk_of_the_best_path():
    for name, lat in MC.all_lattices():
        if not lat.num_nodes:
            continue
        words = lat.best_path()[0]
        start = lat.mbr(max_iterations=0, hypothesis=words)
        res = lat.mbr()
        assert res.risk <= start.risk + RISK_TOL, (name, res, start)
        assert res.iterations >= 1 and len(res.confidence) == len(res.frames) == len(res.words)
        check_sausage(res)
        again = lat.mbr(max_iterations=0, hypothesis=res.words)
        assert again.risk == res.risk and again.confidence == res.confidence and again.sausage == res.sausage


def test_without_words():
    lat = NC.without_words(MC.tree_lattice())
    res = lat.mbr()
    assert res.words == [] and res.risk == 0.0 and res.sausage == [] and res.iterations == 1


def test_the_long_hypothesis_has_more_than_32_words():
    res = LatticeBatch(MC.long_lattices()).mbr()
    assert len(res[0].words) >= 33                  # S + 1 > 64 columns: two rounds of a wave on the device
    assert len(res[1].words) <= 1
    check_sausage(res[0])


def test_empty_and_partial_utterances_keep_their_places():
    from wfst_cases import grid_scores, toy_graph
    import torch
    from att_speech.wfst_lattice import decode_lattice
    g = toy_graph('c')
    lens = [1, 5, 2]
    lp = torch.from_numpy(grid_scores(np.random.default_rng(4), 5, 3, 3, lens, low=-4.0))
    gone = decode_lattice(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=False)[0]
    partial = decode_lattice(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=True)[0]
    assert not gone[0].num_nodes and not gone[2].num_nodes and not partial[0].reached_final
    res = LatticeBatch(gone).mbr()
    assert res[0] == MBR_NONE and res[2] == MBR_NONE and res[0].risk == INF and res[1].risk < INF
    assert res[1] == gone[1].mbr()
    mixed = LatticeBatch([gone[0], gone[1], partial[2]]).mbr()
    assert mixed[0] == MBR_NONE and mixed[1] == res[1] and mixed[2] == partial[2].mbr() and mixed[2].risk < INF
    assert LatticeBatch([_empty(g, 1.0, 3)]).mbr() == [MBR_NONE]
    assert LatticeBatch([]).mbr() == []


def test_twice_the_same_and_given_hypotheses_unchanged():
    lats = NC.unquantised_lattices(4.0)
    batch = LatticeBatch(lats)
    first = batch.mbr()
    assert batch.mbr() == first and all(isinstance(r, MBRResult) for r in first)
    assert [lat.mbr() for lat in lats] == first     # the batch changes nothing
    sents = [lat.sentences(3) for lat in lats]
    for i in range(3):
        hyps = [s[min(i, len(s) - 1)] for s in sents]
        res = batch.mbr(max_iterations=0, hypotheses=hyps)
        assert [r.words for r in res] == hyps and all(r.iterations == 1 for r in res)
    scaled = batch.mbr(0.5, 2.0)
    assert [r.risk for r in scaled] != [r.risk for r in first]
    with pytest.raises(ValueError):
        batch.mbr(hypotheses=[[1]])


def test_conditionals_sum_to_one():
    for name, lat in MC.all_lattices():
        if not lat.num_nodes:
            continue
        hb = LatticeBatch([lat])
        arc, end = hb.conditionals()
        into = np.zeros(lat.num_nodes)
        np.add.at(into, lat.dst, arc)
        has = np.bincount(lat.dst, minlength=lat.num_nodes) > 0
        assert np.allclose(into[has & (into > 0)], 1.0, atol=1e-12), name
        assert abs(end.sum() - 1.0) <= 1e-12
        assert hb.mbr(arc_cond=arc, end_cond=end) == hb.mbr()


def test_the_entry_points_are_exported():
    from att_speech._native import lib
    L = lib()
    assert L.asr_abi_version() == 24
    assert L.asr_lattice_mbr_supported(1000, 5000, 300, 255) == 1
    assert L.asr_lattice_mbr_supported(1000, 5000, 300, 256) == 0
    assert L.asr_lattice_mbr_workspace_bytes(1000, 31) >= 1000 * 16 * 64


def test_device_batch_host_path_and_expected_errors():
    """a DeviceLatticeBatch of CPU tensors runs the twin on a copy, with no launch"""
    from att_speech.lattice_dp import DeviceLatticeBatch
    lats = NC.unquantised_lattices(4.0)
    batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
    host = LatticeBatch(lats)
    assert batch.mbr() == host.mbr() and batch.launches == 0
    assert batch.mbr(0.5, 2.0, max_iterations=3) == host.mbr(0.5, 2.0, max_iterations=3)
    sents = batch.sentences(4)
    risks = batch.expected_errors(sents)
    assert [len(r) for r in risks] == [len(s) for s in sents]
    for b, lat in enumerate(lats):
        assert risks[b] == [lat.mbr(max_iterations=0, hypothesis=s).risk for s in sents[b]]
    with pytest.raises(ValueError):
        batch.expected_errors(sents[:1])


def test_fst_decoder_option():
    import torch
    from grammar_cases import BIGRAM_LM, WSJ_VOCAB
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    kw = dict(normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab, decode_beam=16.0,
              decode_lattice_beam=4.0, decode_nbest=3)
    torch.manual_seed(0)
    plain = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), **kw)
    mbr = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), decode_mbr=True, decode_confidence=True, **kw)
    assert plain.decode_mbr is False and mbr.decode_mbr is True
    mbr.load_state_dict(plain.state_dict())
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    with torch.no_grad():
        want, got = plain.decode(enc, elens), mbr.decode(enc, elens)
    assert 'mbr' not in want and got['decoded'] == want['decoded'] and got['nbest'] == want['nbest']
    assert len(got['mbr']) == len(got['mbr_risk']) == len(got['word_confidence']) == B
    for (words, conf, frames), risk in zip(got['mbr'], got['mbr_risk']):
        assert len(words) == len(conf) == len(frames) and 0.0 <= risk < INF
        assert all(0.0 <= c <= 1.0 + 1e-9 for c in conf) and frames == sorted(frames)
    with pytest.raises(ValueError, match='decode_lattice_beam'):
        FSTDecoder({'features': torch.zeros(B, T, D)}, 49, dict(gg), decode_mbr=True, vocabulary=vocab, decode_beam=16.0)


def test_tool_mbr_flag(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    try:
        import decode_graph as tool
    finally:
        sys.path.pop(0)
    import torch
    from wfst_cases import TOYS
    from att_speech.ctc_forward import KaldiFloatMatrixWriter
    from att_speech.wfst_lattice import decode_lattice
    g, lp = NC.toy_inputs('a')
    utts = [('utt%d' % b, lp[:n, b]) for b, n in enumerate(NC.LENS)]
    ark, fst, out = tmp_path / 'lp.ark', tmp_path / 'g.txt', tmp_path / 'mbr.txt'
    with KaldiFloatMatrixWriter(str(ark)) as writer:
        for key, m in utts:
            writer[key] = m
    t = TOYS['a']
    with open(str(fst), 'w') as f:
        for s, il, ol, w, d in t['arcs']:
            f.write('%d %d %d %d %g\n' % (s, d, il, ol, w))
        for s, w in t['final'].items():
            f.write('%d %g\n' % (s, w))
    tool.main([str(ark), str(fst), '--lattice-beam', '2', '--mbr', str(out), '--device', 'cpu', '--batch', '3'])
    lats, _ = decode_lattice(torch.from_numpy(np.nan_to_num(lp)), NC.LENS, g, beam=16.0, lattice_beam=2.0)
    want = LatticeBatch(lats).mbr()
    assert out.read_text().splitlines() == [' '.join(['utt%d' % b] + [str(w) for w in r.words])
                                            for b, r in enumerate(want)]
    rows = [l.split() for l in (tmp_path / 'mbr.txt.conf').read_text().splitlines()]
    assert rows == [['utt%d' % b, str(w), str(f), '%.6f' % c] for b, r in enumerate(want)
                    for w, f, c in zip(r.words, r.frames, r.confidence)] and len(rows) > 4
    with pytest.raises(SystemExit):
        tool.main([str(ark), str(fst), '--mbr', str(out)])


def test_argument_checks_need_no_gpu():
    """bad sizes and null pointers: the status comes back before any launch"""
    import ctypes
    from att_speech import _native
    L = _native.lib()
    off = (ctypes.c_int64 * 2)(0, 0)
    h = ctypes.cast(off, ctypes.c_void_p)
    one = ctypes.c_void_p(8)                            # never dereferenced: b_count = 0 or refused before

    def call(max_iterations=16, max_words=8, cap=64, init=(None, None), b_count=0):
        return L.asr_lattice_mbr_f64(1, 0, b_count, 0, 0, 0, h, h, h, *[one] * 18, float('nan'), 1.0, 1, 0, one, one,
                                     one, 0, 0, None, None, init[0], init[1], max_iterations, max_words, cap,
                                     *[one] * 11, one, 1024, None)
    assert call() == _native.ASR_OK
    assert call(max_words=0) == _native.ASR_EINVAL and call(max_words=256) == _native.ASR_EUNSUPPORTED
    assert call(max_iterations=-1) == _native.ASR_EINVAL and call(cap=0) == _native.ASR_EINVAL
    assert call(init=(one, None)) == _native.ASR_EINVAL
    assert L.asr_lattice_mbr_workspace_bytes(-1, 8) == 0 and L.asr_lattice_mbr_workspace_bytes(10, 0) == 0
    assert L.asr_lattice_mbr_workspace_bytes(10, 255) >= 10 * (16 * 512 + 8)
