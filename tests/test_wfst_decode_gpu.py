"""asr_wfst_decode_f32 (csrc/wfst_decode.hip) through att_speech.wfst_decode.decode_graph.

Inputs sit on the 2^-8 grid of tests/wfst_cases.py (arc weights, final costs, lp with |lp| <= 32,
beam, acoustic_scale in {1, 0.5}, T <= 64): every fp32 sum is exact, so the device must equal
the fp64 referee (tests/wfst_referee.py) in every field, bit for bit.  Frames beyond an
utterance's length are NaN: a kernel that read them would carry the NaN into its costs."""
import warnings

import numpy as np
import pytest
import torch

import wfst_referee as R
from grammar_cases import BIGRAM_LM, WSJ_VOCAB
from test_lattice_gpu import dev
from wfst_cases import INF, TOYS, assert_same, grid_scores, random_graph, toy_graph

pytestmark = pytest.mark.gpu


def _device(g, lp, lens, **kw):
    from att_speech.wfst_decode import decode_graph
    out = decode_graph(torch.from_numpy(lp).to(dev()), lens, g, **kw)
    assert out['alignment'].is_cuda and out['cost'].dtype == torch.float32
    return out


def _check(g, lp, lens, **kw):
    got = _device(g, lp, lens, **kw)
    assert got['redone_on_host'] == []
    want = R.decode(*R.graph_args(g), lp, lens, **kw)
    assert_same(got, want, str(kw))
    return got, want


@pytest.mark.parametrize('name', sorted(TOYS))
def test_toy_graphs(name):
    g = toy_graph(name)
    lens = [5, 1, 3, 5]
    rng = np.random.default_rng(len(name) + 3)
    lp = grid_scores(rng, 5, 4, 3, lens, low=-4.0)
    for scale in (1.0, 0.5):
        for beam in (INF, 1.0):
            _check(g, lp, lens, beam=beam, acoustic_scale=scale)


def test_switch_selects_the_host_path_per_call(monkeypatch):
    """ASR_WFST_NATIVE=0 on a device tensor: the host path, same bits, fields back on the device"""
    from att_speech import _native
    g = toy_graph('a')
    lens = [5, 1, 3, 5]
    lp = grid_scores(np.random.default_rng(9), 5, 4, 3, lens, low=-4.0)
    native = _device(g, lp, lens, beam=2.0)
    monkeypatch.setenv('ASR_WFST_NATIVE', '0')
    monkeypatch.setattr(_native, 'lib', lambda: pytest.fail('the native library was called'))
    assert_same(_device(g, lp, lens, beam=2.0), native)


def test_fan_out_and_fan_in():
    """One state with 3000 out-arcs (spread over the workgroup by the prefix-sum search) and one
    state entered by 3000 arcs, most of them at equal cost: the smallest arc index must win
    whichever lane gets there first."""
    from att_speech.wfst_decode import DecodingGraph
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
    perm = rng.permutation(len(src))            # arc indices unrelated to the order of the states
    g = DecodingGraph(F + 3, 0, src[perm], dst[perm], il[perm], ol[perm], w[perm], final)
    lens = [4, 3]
    lp = -rng.integers(1, 3, size=(4, 2, C)).astype(np.float32)      # two values only: ties everywhere
    lp[3:, 1] = np.nan
    got, want = _check(g, lp, lens, beam=INF)
    assert want['num_active'].max() >= F
    assert all(len(x) >= 2 for x in got['words'])
    _check(g, lp, lens, beam=0.0)


def test_wide_state_ids():
    """70 000 states: ids beyond 16 bits, epsilon arcs at two ranks"""
    rng = np.random.default_rng(70)
    g = random_graph(rng, 70000, 50, arcs_per_state=4)
    assert g.num_ranks == 2
    lens = [12, 7, 12]
    lp = grid_scores(rng, 12, 3, 50, lens)
    got, want = _check(g, lp, lens, beam=INF)
    assert want['num_active'].max() > 65535
    assert np.isfinite(want['cost']).all()
    _check(g, lp, lens, beam=6.0, acoustic_scale=0.5)


def test_wide_alphabet():
    rng = np.random.default_rng(2401)
    C = 2401
    g0 = random_graph(rng, 600, C, arcs_per_state=6)
    il = g0.ilabel.copy()
    il[g0.ptr[0]] = C                           # the start state reads the last class
    from att_speech.wfst_decode import DecodingGraph
    g = DecodingGraph(g0.num_states, 0, g0.src, g0.dst, il, g0.olabel, g0.weight, g0.final)
    assert g.max_ilabel == C
    lens = [8, 5]
    lp = grid_scores(rng, 8, 2, C, lens)
    lp[0, :, C - 1] = 0.0                       # and that arc is attractive
    _check(g, lp, lens, beam=INF)
    _check(g, lp, lens, beam=4.0)


def test_finite_beam():
    """Seeds picked on the CPU so that beam = 2 changes the referee's answer and removes tokens."""
    picked = None
    for seed in range(40):
        rng = np.random.default_rng(seed)
        g = random_graph(rng, 400, 9, final_share=0.05)
        lens = [14, 9, 14]
        lp = grid_scores(rng, 14, 3, 9, lens)
        full = R.decode(*R.graph_args(g), lp, lens, beam=INF)
        tight = R.decode(*R.graph_args(g), lp, lens, beam=2.0)
        if (tight['cost'] != full['cost']).any() and tight['words'] != full['words'] and \
                (tight['num_active'] < full['num_active']).any():
            picked = (g, lp, lens, tight)
            break
    assert picked is not None
    g, lp, lens, tight = picked
    assert_same(_device(g, lp, lens, beam=2.0), tight)
    _check(g, lp, lens, beam=0.0)
    _check(g, lp, lens, beam=16.0)


@pytest.mark.parametrize('allow_partial', [True, False])
def test_no_final_state_reached(allow_partial):
    g = toy_graph('c')                          # its final state is at least three frames away
    lens = [1, 2, 2]
    lp = grid_scores(np.random.default_rng(4), 2, 3, 3, lens, low=-4.0)
    got, want = _check(g, lp, lens, beam=INF, allow_partial=allow_partial)
    assert not want['reached_final'].any()
    if allow_partial:
        assert np.isfinite(want['cost']).all() and (want['alignment'][:, 0] > 0).all()
    else:
        assert np.isinf(want['cost']).all() and (want['alignment'] == -1).all() and not any(want['words'])


def _redo_case(monkeypatch, g, lp, lens, beam, list_cap, log_cap, exceeded):
    """Run with the given capacities (the plan of the workspace is replaced, nothing else).  Host
    statistics say what utterance 1, and only that one, outgrows: `exceeded` names the capacity.
    It must come back flagged, be redone on the host with one warning, and equal the referee."""
    from att_speech import wfst_decode
    stats = wfst_decode.decode_graph_host(np.nan_to_num(lp), lens, g, beam=beam)['stats']
    word_cap = wfst_decode.word_capacity(lp.shape[0], g.num_ranks)
    over = [dict(emit=s['peak_emit'] > list_cap, closure=s['peak_closure'] > list_cap,
                 log=s['records'] > log_cap, words=s['words'] > word_cap) for s in stats]
    assert not any(over[0].values()) and not any(over[2].values()), over
    assert {k for k, v in over[1].items() if v} == set(exceeded.split('+')), over
    monkeypatch.setattr(wfst_decode, 'plan_workspace', lambda N, T, B, budget: (B, list_cap, log_cap))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        got = _device(g, lp, lens, beam=beam)
    assert len([w for w in rec if 'decode_graph' in str(w.message)]) == 1
    assert got['redone_on_host'] == [1]
    assert_same(got, R.decode(*R.graph_args(g), lp, lens, beam=beam))


def _steered_scores(T, favourite):
    """lp [T, B, 2] on the grid: utterance b prefers class favourite[b] by 8 at every frame"""
    lp = np.full((T, len(favourite), 2), -8.0, np.float32)
    for b, c in enumerate(favourite):
        lp[:, b, c] = -0.25
    return lp


def test_list_overflow_in_the_emitting_phase(monkeypatch):
    """no epsilon arcs at all: the list can only be outgrown by the emitting expansion (the count
    "after the closure" is then the emitting phase's own survivors)"""
    rng = np.random.default_rng(12)
    g = random_graph(rng, 300, 11, eps_share=0.0)
    assert g.num_ranks == 0
    lens = [3, 16, 3]
    lp = grid_scores(rng, 16, 3, 11, lens)
    _redo_case(monkeypatch, g, lp, lens, INF, list_cap=150, log_cap=17 * 300, exceeded='emit+closure')


def test_list_overflow_in_the_first_of_two_epsilon_levels(monkeypatch):
    """A hub whose 600 epsilon arcs (level 0) lead to states that have epsilon arcs of their own
    (level 1).  With 100 list slots level 0 counts past the end of the list; level 1 must not
    read what was never written.  Utterances 0 and 2 prefer class 2 and prune the hub away."""
    from att_speech.wfst_decode import DecodingGraph
    K = 600
    mids = np.arange(10, 10 + K)
    arcs = [(0, 1, 7, 0.0, 1), (0, 2, 0, 0.0, 2), (2, 2, 0, 0.0, 2), (2, 1, 0, 0.5, 2),
            (1, 1, 8, 0.25, 2), (1, 2, 0, 0.25, 2), (3, 1, 9, 0.0, 2), (3, 2, 0, 0.0, 2)]
    src, il, ol, w, dst = [list(x) for x in zip(*arcs)]
    src += [1] * K + mids.tolist()
    dst += mids.tolist() + [3] * K
    il += [0] * (2 * K)
    ol += (mids + 100).tolist() + [0] * K
    w += (np.arange(K) % 4 / 4.0).tolist() + (np.arange(K) % 3 / 8.0).tolist()
    final = np.full(10 + K, INF)
    final[[2, 3]] = [0.5, 0.0]
    g = DecodingGraph(10 + K, 0, src, dst, il, ol, w, final)
    assert g.num_ranks == 2
    lens = [4, 4, 3]
    lp = _steered_scores(4, [1, 0, 1])
    lp[3:, 2] = np.nan
    _redo_case(monkeypatch, g, lp, lens, 0.5, list_cap=100, log_cap=5 * (K + 10), exceeded='closure')


def test_log_overflow(monkeypatch):
    rng = np.random.default_rng(12)
    g = random_graph(rng, 300, 11)
    lens = [3, 16, 3]
    lp = grid_scores(rng, 16, 3, 11, lens)
    _redo_case(monkeypatch, g, lp, lens, INF, list_cap=300, log_cap=1500, exceeded='log')


def test_word_overflow(monkeypatch):
    """a chain of twelve epsilon arcs with a word on each: thirteen words a frame, more than the
    eight a frame the word buffer holds; utterances 0 and 2 stay on a silent loop"""
    from att_speech.wfst_decode import DecodingGraph, word_capacity
    chain = [1] + list(range(3, 15))            # thirteen states, twelve epsilon arcs; 2 is the silent loop
    arcs = [(0, 1, 1, 0.0, 1), (0, 2, 0, 0.0, 2), (2, 2, 0, 0.0, 2), (2, 1, 0, 0.5, 2),
            (14, 1, 1, 0.0, 1), (14, 2, 0, 0.25, 2)]
    arcs += [(chain[k], 0, 101 + k, 0.0, chain[k + 1]) for k in range(12)]    # free: the beam keeps the chain
    src, il, ol, w, dst = [np.array(x) for x in zip(*arcs)]
    final = np.full(15, INF)
    final[[2, 14]] = 0.0
    g = DecodingGraph(15, 0, src, dst, il, ol, w, final)
    assert g.num_ranks == 12 and word_capacity(4, g.num_ranks) == 40
    lens = [4, 4, 2]
    lp = _steered_scores(4, [1, 0, 1])
    lp[2:, 2] = np.nan
    _redo_case(monkeypatch, g, lp, lens, 0.5, list_cap=15, log_cap=5 * 15, exceeded='words')


def test_tables_beyond_the_budget_run_in_chunks():
    from att_speech.wfst_decode import plan_workspace
    rng = np.random.default_rng(13)
    g = random_graph(rng, 5000, 11)
    lens = [6, 4, 6, 5, 6]
    lp = grid_scores(rng, 6, 5, 11, lens)
    budget = 12 * 5000 * 4 + 4096               # tables of two utterances take half of it
    assert plan_workspace(5000, 6, 5, budget)[0] == 2
    got = _device(g, lp, lens, beam=3.0, workspace_bytes=budget)
    assert_same(got, R.decode(*R.graph_args(g), lp, lens, beam=3.0))


def _bigram_generator():
    from att_speech import fst_utils as P
    return P.CTCGraphGen(context_order=1, num_symbols=49, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)


def test_shipped_bigram_lm_against_fst_decoder():
    """mono o bigram (194 states) through from_graph_generator, beam = inf: the labels of
    FSTDecoder.decode, and the referee's cost within 6 T 2^-24 sum |terms on the fp64 best path|.
    The seed is chosen on the CPU so that, for the referee, the best label sequence beats every
    other label sequence by more than 1e-3: far more than fp32 rounding can move a path's cost, so
    the two fp32 searches must return the same labels."""
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    from att_speech.wfst_decode import DecodingGraph, decode_graph
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    elens = torch.tensor([16, 11], dtype=torch.int32)
    dec = FSTDecoder({'features': torch.zeros(B, T, D)}, 49,
                     dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM,
                          vocabulary=WSJ_VOCAB),
                     normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab)
    dg = DecodingGraph.from_graph_generator(dec.graph_generator)
    assert dg.num_states == 194 and dg.num_ranks == 0
    dec.to(dev())
    picked = None
    for seed in range(10):      # the scores are the decoder's own logits; the referee judges them on the CPU
        torch.manual_seed(seed)
        enc = torch.randn(T, B, D) * 3
        with torch.no_grad():
            out = dec.decode(enc.to(dev()), elens)
        logits = out['logits'].cpu().numpy()
        ref = R.decode(*R.graph_args(dg), logits, elens.tolist(), beam=INF)
        gaps = [R.best_other_words_cost(*R.graph_args(dg), logits[:, b], int(elens[b]), ref['words'][b])
                - ref['cost'][b] for b in range(B)]
        assert min(gaps) >= 0
        if min(gaps) > 1e-3 and all(len(w) >= 2 for w in ref['words']):
            picked = (out, ref)
            break
    assert picked is not None
    out, ref = picked
    got = decode_graph(out['logits'], elens, dg, beam=INF)
    assert got['words'] == out['decoded'] == ref['words']
    assert (got['alignment'].cpu().numpy() == ref['alignment']).all()
    bound = 6 * T * 2.0 ** -24 * ref['abs_terms']
    assert (np.abs(got['cost'].cpu().numpy().astype(np.float64) - ref['cost']) <= bound).all()


def test_fst_decoder_decode_beam():
    """FSTDecoder(decode_beam=16) on the bigram-context generator (S = 49, C = 2401): the labels
    of the default path."""
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 12, 16
    gg = dict(class_name='CTCGraphGen', context_order=2, graph_build_args=dict(use_contextual_blanks=True))
    torch.manual_seed(1)
    exact = FSTDecoder({'features': torch.zeros(B, T, D)}, 2401, graph_generator=gg, vocabulary=vocab)
    beamed = FSTDecoder({'features': torch.zeros(B, T, D)}, 2401, graph_generator=gg, vocabulary=vocab,
                        decode_beam=16.0)
    assert exact.decode_beam is None
    beamed.load_state_dict(exact.state_dict())
    exact.to(dev())
    beamed.to(dev())
    enc = (torch.randn(T, B, D) * 2).to(dev())
    elens = torch.tensor([12, 9], dtype=torch.int32)
    with torch.no_grad():
        want = exact.decode(enc, elens)['decoded']
        got = beamed.decode(enc, elens)['decoded']
    assert got == want and all(len(w) >= 1 for w in want)


def test_unquantised_scores_match_the_host_path_bit_for_bit():
    from att_speech.wfst_decode import DecodingGraph, decode_graph
    rng = np.random.default_rng(40)
    g0 = random_graph(rng, 3000, 40, arcs_per_state=5)
    w = rng.standard_normal(len(g0.src)).astype(np.float32) + np.float32(0.7)
    fin = np.where(np.isfinite(g0.final), rng.random(g0.num_states).astype(np.float32), np.float32(INF))
    g = DecodingGraph(g0.num_states, 0, g0.src, g0.dst, g0.ilabel, g0.olabel, w, fin)
    T, B = 40, 8
    lens = rng.integers(T // 2, T + 1, size=B)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, B, 40)).astype(np.float32) * 3), -1)
    for scale in (1.0, 0.3):
        got = decode_graph(lp.to(dev()), lens, g, beam=16.0, acoustic_scale=scale)
        want = decode_graph(lp, lens, g, beam=16.0, acoustic_scale=scale)
        assert got['redone_on_host'] == [] and got['words'] == want['words']
        for k in ('alignment', 'reached_final', 'num_active'):
            assert torch.equal(got[k].cpu(), want[k]), k
        assert torch.equal(got['cost'].cpu().view(torch.int32), want['cost'].view(torch.int32))
        assert np.isfinite(want['cost'].numpy()).all() and int(want['num_active'].max()) > 100
