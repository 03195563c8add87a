"""LatticeBatch.oracle (att_speech/wfst_lattice.py), the numpy twin of asr_lattice_oracle_i32, against ground
truth: the least Levenshtein distance over every complete path of lattices small enough to enumerate, and on
every case lattice the consistency of the counts, the words, the alignment and the cost with one another."""
import numpy as np
import pytest

import lm_rescore_cases as LC
import mbr_cases as MC
import nbest_cases as NC
from wfst_cases import INF, TOYS

from att_speech.wfst_lattice import (ORACLE_NONE, LatticeBatch, OracleResult, _empty, _oracle_path,
                                     oracle_error_rate)


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]


def brute_lattices():
    out = list(MC.enumerable())
    for k in range(3):
        out += [('brute %d #%d' % (k, b), lat) for b, lat in enumerate(LC.brute_case(k)[1])]
    return out


def references(lat, seed):
    """mbr_cases' probes and seeded random references of 1, 3 and 7 labels"""
    rng = np.random.default_rng(seed)
    top = int(lat.graph.olabel.max()) + 2
    return [list(h) for h in MC.probe_hypotheses(lat)] + [rng.integers(1, top + 1, n).tolist() for n in (1, 3, 7)]


def check_consistent(lat, ref, res, what):
    """everything a result promises about itself"""
    assert isinstance(res, OracleResult) and res != ORACLE_NONE, what
    R = len(ref)
    assert res.substitutions + res.insertions + res.deletions == res.errors, what
    assert res.correct + res.substitutions + res.deletions == R, what
    assert min(res.substitutions, res.insertions, res.deletions, res.correct) >= 0, what
    assert levenshtein(res.words, ref) == res.errors, what
    assert len(res.ref_frames) == R and sum(1 for f in res.ref_frames if f == -1) == res.deletions, what
    kept = [f for f in res.ref_frames if f >= 0]
    assert all(f >= -1 for f in res.ref_frames) and kept == sorted(kept), what
    assert all(f <= lat.num_frames for f in kept), what       # 0: a word on a non-emitting arc at the start
    assert (res.words, res.cost) == rewalk(lat, ref), what


def rewalk(lat, ref):
    """(words, cost at the lattice's own scales) of the twin's path, re-walked arc by arc: it must lead from
    the start node to an end node, every arc leaving where the last one arrived"""
    g = lat.graph
    path, last = _oracle_path(lat, [int(w) for w in ref])[3:]
    v = int(np.nonzero((lat.time == 0) & (lat.state == g.start))[0][0])
    total, words = np.float64(0.0), []
    for j in path:
        assert lat.src[j] == v
        v = int(lat.dst[j])
        x = np.float64(1.0) * np.float64(g.weight[lat.arc[j]]) - np.float64(lat.acoustic_scale) * np.float64(lat.lp[j])
        total = total + x
        if g.olabel[lat.arc[j]] != 0:
            words.append(int(g.olabel[lat.arc[j]]))
    assert v == last and lat.time[v] == lat.num_frames
    end = np.float64(0.0)
    if lat.reached_final:
        assert g.final[lat.state[v]] < INF
        end = np.float64(1.0) * np.float64(g.final[lat.state[v]])
    return words, float(total + end)


@pytest.mark.parametrize('name,lat', brute_lattices(), ids=[n for n, _ in brute_lattices()])
def test_against_every_path(name, lat):
    """errors == the least Levenshtein distance over all complete paths; nothing is skipped as TooManyPaths"""
    paths = LC.complete_paths(lat)
    sentences = {tuple(LC.path_words(lat, p)) for p in paths}
    for ref in references(lat, len(name)):
        res = lat.oracle(ref)
        if not paths:
            assert res == ORACLE_NONE, (name, ref)
            continue
        assert res.errors == min(levenshtein(s, ref) for s in sentences), (name, ref, res)
        assert tuple(res.words) in sentences, (name, ref)
        check_consistent(lat, ref, res, (name, ref))


def test_all_brute_cases_enumerate():
    counts = [len(LC.complete_paths(lat)) for _, lat in brute_lattices()]
    assert len(counts) == 135 and max(counts) == 1594


def test_an_empty_lattice_has_no_oracle():
    g = NC.toy_inputs('a')[0]
    assert _empty(g, 1.0, 3).oracle([1, 2]) == ORACLE_NONE
    assert LatticeBatch([_empty(g, 1.0, 3), MC.single_path()]).oracle([[1], [3, 4, 4, 2]])[0] == ORACLE_NONE
    assert LatticeBatch([]).oracle([]) == []


def big_lattices():
    return [('fan', NC.fan_lattice()), ('long', MC.long_lattices()[0])] + \
        [('unquantised #%d' % b, lat) for b, lat in enumerate(NC.unquantised_lattices(4.0))]


@pytest.mark.parametrize('name,lat', big_lattices(), ids=[n for n, _ in big_lattices()])
def test_consistency_on_the_large_cases(name, lat):
    sents = lat.sentences(3)
    rng = np.random.default_rng(7)
    refs = [list(s) for s in sents] + [[], sents[0][::-1], sents[-1] + [5, 5], sents[0][1:-1],
                                       rng.integers(1, 30, 9).tolist()]
    best = lat.best_path()[0]
    for ref in refs:
        res = lat.oracle(ref)
        check_consistent(lat, ref, res, (name, ref))
        assert res.errors <= levenshtein(best, ref), (name, ref)


@pytest.mark.parametrize('name,lat', MC.all_lattices(), ids=[n for n, _ in MC.all_lattices()])
def test_a_sentence_of_the_lattice_is_found_exactly(name, lat):
    if not lat.num_nodes:
        return
    best = lat.best_path()[0]
    for words, _ in lat.nbest(5):
        res = lat.oracle(words)
        assert res.errors == 0 and res.words == list(words), (name, words, res)
        assert res.correct == len(words) and res.insertions == res.deletions == res.substitutions == 0
        assert all(f >= 0 for f in res.ref_frames)
    for ref in references(lat, 3):
        assert lat.oracle(ref).errors <= levenshtein(best, ref), (name, ref)


@pytest.mark.parametrize('name', sorted(TOYS))
def test_errors_never_rise_with_the_lattice_beam(name):
    rng = np.random.default_rng(2)
    refs = [rng.integers(1, 6, n).tolist() for n in (0, 1, 2, 4, 6)]
    for scale in NC.SCALES:
        for ref in refs:
            last = None
            for lb in NC.LATTICE_BEAMS:
                lats = NC.toy_lattices(name, scale, lb)[0]
                errs = [r.errors for r in LatticeBatch(lats).oracle([ref] * len(lats))]
                if last is not None:
                    assert all(e <= l for e, l in zip(errs, last) if l >= 0), (name, scale, lb, ref, errs, last)
                    assert all(e >= 0 for e, l in zip(errs, last) if l >= 0)
                last = errs


@pytest.mark.parametrize('name,lat', brute_lattices()[:40], ids=[n for n, _ in brute_lattices()[:40]])
def test_the_empty_reference_finds_the_fewest_words(name, lat):
    paths = LC.complete_paths(lat)
    if not paths:
        return
    res = lat.oracle([])
    fewest = min(len(LC.path_words(lat, p)) for p in paths)
    assert res.errors == res.insertions == len(res.words) == fewest and res.ref_frames == []


def test_reference_labels_must_be_positive():
    lat = MC.single_path()
    for ref in ([0], [3, -1], [3, 0, 4]):
        with pytest.raises(ValueError):
            lat.oracle(ref)
    with pytest.raises(ValueError):
        LatticeBatch([lat]).oracle([[1], [2]])


def test_scales_change_the_cost_alone():
    lat = NC.unquantised_lattices(4.0)[0]
    ref = lat.sentences(2)[-1]
    a, b = lat.oracle(ref), lat.oracle(ref, 0.5, 2.0)
    assert a[:7] == b[:7] and a.cost != b.cost
    assert a.cost == lat.oracle(ref, lat.acoustic_scale, 1.0).cost


def test_depth_is_a_direct_count():
    lats = NC.unquantised_lattices(4.0) + [_empty(NC.bigram_graph(), 1.0, 4)]
    want = []
    for lat in lats:
        n = sum(1 for j in range(lat.num_arcs) if lat.graph.ilabel[lat.arc[j]] != 0)
        want.append(n / lat.num_frames if lat.num_nodes else 0.0)
    assert LatticeBatch(lats).depth() == want and want[-1] == 0.0 and want[0] > 1.0
    assert [lat.depth() for lat in lats] == want


def test_oracle_error_rate():
    lats = [MC.single_path(), _empty(MC.single_path().graph, 1.0, 2), MC.single_path()]
    refs = [[3, 4, 2], [1, 1], [3, 4, 4, 2, 9]]
    res = LatticeBatch(lats).oracle(refs)
    assert [r.errors for r in res] == [1, -1, 1]
    rate = oracle_error_rate(res, refs)
    assert tuple(rate) == (2, 8, 0.25, 1) and rate.skipped == 1
    assert tuple(oracle_error_rate([], [])) == (0, 0, 0.0, 0)


def test_a_device_batch_of_cpu_tensors_takes_the_twin():
    from att_speech.lattice_dp import DeviceLatticeBatch
    lats = NC.unquantised_lattices(4.0) + [_empty(NC.bigram_graph(), 1.0, 4)]
    batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
    host = LatticeBatch(lats)
    refs = [lat.sentences(1)[0][1:] + [7] if lat.num_nodes else [3] for lat in lats]
    assert batch.oracle(refs) == host.oracle(refs) and batch.launches == 0
    assert batch.oracle(refs, 0.5, 2.0) == host.oracle(refs, 0.5, 2.0)
    assert batch.oracle(refs)[-1] == ORACLE_NONE
    assert batch.depth() == host.depth()
    with pytest.raises(ValueError):
        batch.oracle(refs[:-1])
    with pytest.raises(ValueError):
        batch.oracle([[0]] * len(lats))


def test_the_native_entries_refuse_what_they_cannot_hold():
    from att_speech import _native
    L = _native.lib()
    assert L.asr_lattice_oracle_supported(1000, 5000, 300, 1023) == 1
    assert L.asr_lattice_oracle_supported(1000, 5000, 300, 1024) == 0
    assert L.asr_lattice_oracle_supported(1000, 5000, 300, 0) == 0
    assert L.asr_lattice_oracle_supported(2 ** 30, 5000, 2 ** 30 - 1000, 1023) == 0    # levels + words reach 2^30
    assert L.asr_lattice_oracle_workspace_bytes(1000, 63) >= 1000 * 4 * 64
    assert L.asr_lattice_oracle_workspace_bytes(-1, 8) == 0 and L.asr_lattice_oracle_workspace_bytes(10, 1024) == 0


def test_fst_decoder_wants_a_lattice_for_the_oracle():
    import torch
    from grammar_cases import BIGRAM_LM, WSJ_VOCAB
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    kw = dict(normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab, decode_beam=16.0)
    sample = {'features': torch.zeros(2, 16, 24)}
    with pytest.raises(ValueError, match='decode_lattice_beam'):
        FSTDecoder(sample, 49, dict(gg), decode_oracle=True, **kw)
    torch.manual_seed(0)
    dec = FSTDecoder(sample, 49, dict(gg), decode_oracle=True, decode_lattice_beam=4.0, **kw)
    flagless = FSTDecoder(sample, 49, dict(gg), decode_lattice_beam=4.0, **kw)
    flagless.load_state_dict(dec.state_dict())
    dec._utterance_losses = flagless._utterance_losses = lambda *a, **k: torch.zeros(2)   # the loss has no CPU path
    enc = torch.randn(16, 2, 24) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    texts = torch.tensor([[5, 9, 12, 7, 3, 0], [20, 4, 4, 8, 0, 0]], dtype=torch.int32)
    tlens = torch.tensor([5, 4], dtype=torch.int32)
    with torch.no_grad():
        got = dec.decode(enc, elens, texts, tlens)
        assert 'oracle' not in dec.decode(enc, elens) and 'oracle' not in flagless.decode(enc, elens, texts, tlens)
    assert got['decoded'] == flagless.decode(enc, elens)['decoded']
    for b, (errors, words) in enumerate(got['oracle']):
        ref = texts[b, :int(tlens[b])].tolist()
        assert errors == levenshtein(words, ref) <= levenshtein(got['decoded'][b], ref)


def test_the_tool_writes_the_oracle(tmp_path):
    import os
    import sys
    import torch
    import wfst_cases as WC
    from att_speech.lattice_dp import decode_lattice_device
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        import decode_graph as tool
    finally:
        sys.path.pop(0)
    g, lats, lm = LC.brute_case(0)
    seed, N, T, lens, beam, lb, fs = LC.BRUTE[0]
    rng = np.random.default_rng(seed)
    WC.random_graph(rng, N, 3, final_share=fs, n_words=LC.N_WORDS)      # the draws of brute_case, in its order
    lp = WC.grid_scores(rng, T, len(lens), 3, lens, low=-4.0)
    utts = [('utt%d' % b, lp[:n, b]) for b, n in enumerate(lens)]
    refs = {'utt%d' % b: [1 + (b + k) % LC.N_WORDS for k in range(b + 2)] for b in range(len(lens))}
    ref_file = tmp_path / 'ref.txt'
    ref_file.write_text(''.join(' '.join([k] + [str(w) for w in r]) + '\n' for k, r in refs.items()))
    assert tool.read_references(str(ref_file)) == refs
    rescore = tool.make_rescorer(lm, beam=2.0)
    for name, kw in (('plain', {}), ('rescored', dict(rescore=rescore))):
        out = tmp_path / (name + '.txt')
        tool.write_oracle(g, utts, str(out), refs, beam=beam, lattice_beam=lb, batch=3, **kw)
        batch, _ = decode_lattice_device(torch.from_numpy(np.nan_to_num(lp)), lens, g, beam=beam, lattice_beam=lb)
        batch = batch.rescore_lm(lm, lattice_beam=2.0) if kw else batch
        order = [refs['utt%d' % b] for b in range(len(lens))]
        want, depth = batch.oracle(order), batch.depth()
        rows = [' '.join(['utt%d' % b] + [str(v) for v in (r.errors, r.substitutions, r.insertions, r.deletions,
                                                          len(order[b]))] + ['%.6f' % depth[b]]
                         + [str(w) for w in r.words]) for b, r in enumerate(want)]
        total = oracle_error_rate(want, order)
        rows.append('TOTAL %d %d %.6f %.6f' % (total.errors, total.reference_words, total.rate, np.mean(depth)))
        assert out.read_text().splitlines() == rows and total.reference_words > 0
    with pytest.raises(SystemExit):
        tool.main(['a.ark', 'g.fst', '--oracle', 'ref.txt', '--oracle-out', 'o.txt'])
    with pytest.raises(SystemExit):
        tool.main(['a.ark', 'g.fst', '--lattice-beam', '2', '--oracle', 'ref.txt'])
