"""The fp64 referee of the device graph search (tests/graph_search_referee.py), proved on the CPU:
  * chained behind lm_beam_referee's step it replays the GraphSearch trajectory of
    tests/golden/beam_lm.npz, which is pinned to the reference's own class (letters, maps, gs_V and
    gs_E exactly, scores to 1e-5), with every decision margin above MARGIN_FLOOR;
  * it equals the host GraphSearch on seeded random trajectories;
  * each single-term mutant is told apart on at least one crafted case;
  * the new symbols are exported and refuse bad arguments before launching; the gate of
    AttentionDecoderTCN opens only with ASR_GRAPH_SEARCH_NATIVE=1."""
import os

import numpy as np
import pytest
import torch

import decode_referee as dr
import graph_search_referee as gr
import lm_beam_referee as lr

GOLDEN = np.load(os.path.join(lr.GOLDEN, 'beam_lm.npz'))


def golden_search():
    g = GOLDEN
    # (the golden search was driven for all 11 steps, past the step that filled its finished list: the
    # host class has no freeze, so the step referee runs with lm_beam_referee's `frozen_still_updating`)
    rs = gr.RefGraphSearch(2, 0.3, lr.toy_lm(), g['mapping'].tolist(), 1, 4, 7, 12, [12], g['logits'].shape[0] + 1,
                           mut='frozen_still_updating')
    for i in range(g['logits'].shape[0]):
        out, _ = rs.step(g['logits'][i][0].astype(np.float64), np.ascontiguousarray(g['att'][i].T.astype(np.float64)))
        np.testing.assert_array_equal(out['new_input'], g['gs_letters'][i])
        np.testing.assert_array_equal(out['parent'], g['gs_maps'][i])
        np.testing.assert_allclose(rs.scores, g['gs_scores'][i], rtol=1e-5)
    return rs


def test_golden_trajectory_is_replayed():
    g = GOLDEN
    rs = golden_search()
    G = gr.merge_graphs_of(rs.store, 0, gr.hash_dec_of(2), 12)
    V, Vs, E = gr.graph_arrays(G)
    np.testing.assert_array_equal(V, g['gs_V'])
    np.testing.assert_array_equal(E, g['gs_E'])
    np.testing.assert_allclose(Vs, g['gs_V_scores'], rtol=1e-5)
    assert int(E[:, 2].sum()) == 5 and int(V[:, 2].sum()) == 10 and rs.events['drops'] + rs.events['old_wins'] > 0
    assert min(lr.min_margin(m) for m in rs.margins) > dr.MARGIN_FLOOR
    sums = min(m['min_sum'] for m in rs.merge_margins)
    scores = min(m['score'] for m in rs.merge_margins)
    print('smallest min-sum margin %.3g, smallest score margin %.3g' % (sums, scores))
    assert sums > dr.MARGIN_FLOOR and scores > dr.MARGIN_FLOOR
    assert rs.events['old_wins'] + rs.events['new_wins'] == 5


# seeds scanned on the CPU for margins above MARGIN_FLOOR along the whole trajectory and at least one merge
RANDOM = [(3, 0, 0.5, 22), (4, 1, 0.5, 20), (4, 2, 0.5, 43), (3, 2, 0.0, 4), (4, 1, 0.0, 21)]


@pytest.mark.parametrize('beam,span,lm_weight,seed', RANDOM)
def test_referee_equals_the_host_class_on_random_trajectories(beam, span, lm_weight, seed):
    from att_speech.modules.beam_search import GraphSearch
    C, T, steps, thr = 7, 12, 10, 0.5
    logits, att = gr.traj_inputs(1, beam, C, steps, seed, [T], T)
    lm, mapping, p = lr.toy_lm(), lr.TOY_MAPPING, lr.PARAMS
    host = GraphSearch(gr.hash_dec_of(span), thr, lm, lm_weight, mapping, p['min_attention_pos'], p['coverage_tau'],
                       p['coverage_weight'], 1, beam, torch.device('cpu'), C, lr.LN, keep_eos_score=False)
    rs = gr.RefGraphSearch(span, thr, lm, mapping, 1, beam, C, T, [T], steps + 1, lm_weight=lm_weight)
    for s in range(steps):
        letters, maps = host.step(torch.from_numpy(logits[s])[None].clone(), att_weights=torch.from_numpy(att[s].T.copy()))
        out, _ = rs.step(logits[s].astype(np.float64), att[s].astype(np.float64))
        np.testing.assert_array_equal(out['new_input'], letters.numpy())
        np.testing.assert_array_equal(out['parent'], maps.numpy())
        np.testing.assert_allclose(rs.scores, host.scores.numpy(), rtol=1e-5, atol=1e-5)   # (the host runs in fp32)
        assert np.isfinite(rs.scores).any()                            # (torch.topk's order among -inf is unspecified)
        if host.has_finished():
            assert rs.state['frozen'][0]
            break
    V, Vs, E = gr.graph_arrays(gr.merge_graphs_of(rs.store, 0, gr.hash_dec_of(span), T))
    hV, hVs, hE = gr.graph_arrays(host.get_graph()[0])
    np.testing.assert_array_equal(V, hV)
    np.testing.assert_array_equal(E, hE)
    np.testing.assert_allclose(Vs, hVs, rtol=1e-5, atol=1e-5)
    assert rs.events['old_wins'] + rs.events['new_wins'] > 0            # something merged
    assert min(gr.min_margin(m) for m in rs.merge_margins) > dr.MARGIN_FLOOR
    assert min(lr.min_margin(m) for m in rs.margins) > dr.MARGIN_FLOOR


def _differs(a, b):
    for k in gr.NODE_KEYS + ('scores', 'tot'):
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True):
            return True
    return False


def test_crafted_cases_hold_what_they_claim_and_tell_the_mutants_apart():
    cases = gr.merge_cases()
    want = {k: gr.merge_ref(c) for k, c in cases.items()}
    ev = want['span2'][2]
    for k in ('empty_buckets', 'dead_candidates', 'lm_state_mismatches', 'below_threshold', 'old_wins', 'new_wins',
              'drops', 'alias_rewrites', 'dead_slots', 'finished_marks'):
        assert ev[k] > 0, k
    assert want['tie'][2]['ties'] > 0 and want['tie'][1]['score'] == 0.0
    assert want['no_lm_term'][2]['lm_state_mismatches'] == 0
    assert want['big'][2]['old_wins'] > 0 and want['big'][2]['new_wins'] > 0 and want['big'][2]['dead_candidates'] > 0
    for k, (_, m, _) in want.items():
        assert m['min_sum'] > dr.MARGIN_FLOOR, k
        if k != 'tie':
            assert m['score'] > dr.MARGIN_FLOOR, k
    # the span changes the buckets
    assert _differs(want['span0'][0], gr.merge_ref(dict(cases['span0'], span=2))[0])
    assert _differs(want['span_longer_than_history'][0], gr.merge_ref(dict(cases['span_longer_than_history'], span=2))[0])
    for mut in gr.MUTANTS:
        caught = [k for k, c in cases.items() if _differs(want[k][0], gr.merge_ref(c, mut)[0])]
        assert caught, mut


def test_symbols_and_argument_checks():
    from att_speech import _native
    L = _native.lib()
    for name in ('asr_beam_lm_step_graph_f32', 'asr_graph_merge_f32', 'asr_graph_search_supported'):
        assert hasattr(L, name) and name in _native._SIGNATURES
    assert L.asr_abi_version() == 24
    assert _native.graph_search_supported(32, 0, 8160) and _native.graph_search_supported(10, 7, 334)
    assert not _native.graph_search_supported(33, 2, 12) and not _native.graph_search_supported(4, -1, 12)
    assert not _native.graph_search_supported(4, 2, 8161) and not _native.graph_search_supported(4, 2, 12, 16)
    p = 0x1000          # a non-null dummy address: every check must fire before anything is launched

    def merge(att=p, bag_state=p, bag_n=p, bag_cap=32, step=3, B=3, beam=4, T=12, Lcap=12, span=2, Ncap=44,
              tot=p + 64, est_out=p + 64, uplink=p):
        return L.asr_graph_merge_f32(att, p, p, tot, p, est_out, p, bag_state, bag_n, bag_cap, p, p, step, B, beam,
                                     T, Lcap, span, 0.5, Ncap, p, p, p, p, p, p, p, p, uplink, None)
    for bad in (dict(att=None), dict(uplink=None), dict(B=0), dict(beam=0), dict(T=0), dict(step=-1), dict(Lcap=3),
                dict(span=-1), dict(Ncap=0), dict(Ncap=15), dict(bag_n=None), dict(tot=p), dict(est_out=p)):
        assert merge(**bad) == _native.ASR_EINVAL, bad
    for bad in (dict(beam=33, Ncap=400), dict(T=8161), dict(bag_cap=16)):
        assert merge(**bad) == _native.ASR_EUNSUPPORTED, bad

    def step(fin_mask=p, tot_out=p + 64, beam=4):
        return L.asr_beam_lm_step_graph_f32(p, p, p, p, 0.5, p, p + 32, p, p + 32, p, p + 32, None, 1, 3, beam, 7, 12, 12,
                                            1.0, 0.3, 0.1, 0.2, p, p, p, p, p, p, p, p, p, p, p, p, p, p,
                                            fin_mask, tot_out, None)
    assert step(fin_mask=None) == _native.ASR_EINVAL and step(tot_out=None) == _native.ASR_EINVAL
    assert step(tot_out=p + 32) == _native.ASR_EINVAL                    # tot_out aliases scores_out
    assert step(beam=33) == _native.ASR_EUNSUPPORTED


class _FakeCuda(object):
    is_cuda, dtype = True, torch.float32

    def __init__(self, T=20, B=2):
        self.shape = (T, B, 16)
        self.device = torch.device('cpu')

    def size(self, i):
        return self.shape[i]


class _FakeLm(object):
    ilabel = np.array([1, 2, 3])

    def eps_rank(self):
        return np.zeros(4, np.int64)

    def device_arrays(self, device):
        return {}


def test_gate(monkeypatch):
    from att_speech.modules.tcn import AttentionDecoderTCN
    for name in ('ASR_TCN_NATIVE', 'ASR_TCN_FF_NATIVE', 'ASR_LM_BEAM_NATIVE', 'ASR_GRAPH_SEARCH_NATIVE'):
        monkeypatch.delenv(name, raising=False)
    dec = AttentionDecoderTCN({'features': torch.zeros(20, 2, 16)}, 6, tcn_hidden_size=24, att_hidden_size=8,
                              dropout_p=0.0, kernel_size=3, dilation_sizes=[1, 2], beam_size=3,
                              vocabulary=['<pad>', '<unk>', ' ', 'a', 'b', 'c'], use_graph_search=True,
                              att_force_forward=(-10, 50)).eval()
    dec.lm, dec.lm_weight = _FakeLm(), 0.5
    batch, single = _FakeCuda(), _FakeCuda(B=1)
    assert not dec._native_lm_ok(batch) and not dec._native_decode_ok(batch)       # off by default
    monkeypatch.setenv('ASR_GRAPH_SEARCH_NATIVE', '1')
    assert dec._native_lm_ok(batch) and dec._native_decode_ok(batch)
    assert dec._native_lm_ok(single) and dec._native_decode_ok(single)             # a single utterance too
    monkeypatch.setenv('ASR_LM_BEAM_NATIVE', '0')
    assert not dec._native_lm_ok(batch) and not dec._native_lm_ok(single)
    monkeypatch.delenv('ASR_LM_BEAM_NATIVE')
    monkeypatch.setenv('ASR_TCN_NATIVE', '0')
    assert not dec._native_decode_ok(batch)
    monkeypatch.delenv('ASR_TCN_NATIVE')
    assert not dec._native_lm_ok(_FakeCuda(T=8161))                                # beyond the merge kernel's frames
    dec.rescore = [3, 4]
    assert not dec._native_lm_ok(batch)
    dec.rescore = None
    monkeypatch.setenv('ASR_GRAPH_SEARCH_NATIVE', '0')
    assert not dec._native_lm_ok(batch)
    # a model without the graph search is untouched by the switch
    dec.use_graph_search = False
    assert dec._native_lm_ok(batch) and not dec._native_lm_ok(single)
    monkeypatch.setenv('ASR_GRAPH_SEARCH_NATIVE', '1')
    assert dec._native_lm_ok(batch) and not dec._native_lm_ok(single)
