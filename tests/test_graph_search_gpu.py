"""The device graph search (asr_beam_lm_step_graph_f32, asr_graph_merge_f32, DeviceGraphSearch,
AttentionDecoderTCN.decode with use_graph_search and ASR_GRAPH_SEARCH_NATIVE=1) against the fp64
referee of tests/graph_search_referee.py, proved on the CPU by tests/test_graph_search_referee.py.

Integer outputs are bit-equal to the referee; every case is seeded so that each decision has a
margin above decode_referee.MARGIN_FLOOR (asserted) or is an exact tie.  The fp32 error of a min-sum
of T <= 130 terms <= 1 is below 1e-5, well inside the margin.  The merge launch only copies scores
(4 fp32 ulps of the largest are allowed); the scores that come out of the step entry follow the rule
of lm_beam_referee.tolerance."""
import os

import numpy as np
import pytest
import torch

import decode_referee as dr
import graph_search_referee as gr
import lm_beam_referee as lr
from test_lm_beam_gpu import DEV, buffers, collect, native, t

pytestmark = pytest.mark.gpu
INF = float('inf')


# ---------------------------------------------------------------- 1. one merge launch from arbitrary state

def merge_buffers(c):
    d = {k: t(v) for k, v in c['store'].items()}
    bags = None
    if c['bags'] is not None:
        bags = tuple(t(x) for x in lr.bags_to_arrays(c['bags']))
    d.update(att=t(c['att'], torch.float32), lens=t(c['lens']), scores=t(c['scores'], torch.float32),
             tot=t(c['tot'], torch.float32), est_in=t(c['est_in']), est_out=t(c['est_out']), fin_mask=t(c['fin_mask']),
             nsteps=t(c['nsteps']), len_pow=t(gr.len_pow(c['est_in'].shape[1], c['length_normalization'])), bags=bags)
    return d


def merge_launch(c, d, **kw):
    a = dict(c, **kw)
    native().graph_merge(d['att'], d['lens'], d['scores'], d['tot'], d['est_in'], d['est_out'], d['fin_mask'],
                         d['bags'], d['nsteps'], d['len_pow'], a['step'], a['B'], a['beam'], a['span'],
                         a['merge_threshold'], {k: d[k] for k in gr.NODE_KEYS})
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in gr.NODE_KEYS + ('scores', 'tot')}


def copy_tol(c):
    s = np.concatenate([np.asarray(c['tot'], np.float64).ravel(), np.asarray(c['store']['node_score'], np.float64).ravel()])
    return 4 * dr.EPS32 * float(np.abs(s[np.isfinite(s)]).max(initial=1.0))


@pytest.mark.parametrize('name', [k for k in gr.merge_cases() if k != 'tie'])
def test_merge_from_arbitrary_state(name):
    c = gr.merge_cases()[name]
    want, margins, ev = gr.merge_ref(c)
    assert gr.min_margin(margins) > dr.MARGIN_FLOOR
    got = merge_launch(c, merge_buffers(c))
    print('%s smallest margins %s events %s' % (name, margins, dict(ev)))
    assert gr.judge_merge(c, got, want, copy_tol(c)) == []
    again = merge_launch(c, merge_buffers(c))                     # repeatable bit for bit
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


# ---------------------------------------------------------------- 2. an exact tie

def test_exact_tie_goes_to_the_old_branch():
    c = gr.merge_cases()['tie']
    want, margins, ev = gr.merge_ref(c)
    assert margins['score'] == 0.0 and ev['ties'] == 2 and margins['min_sum'] > dr.MARGIN_FLOOR
    got = merge_launch(c, merge_buffers(c))
    assert gr.judge_merge(c, got, want, copy_tol(c)) == []
    for b in (0, 2):
        assert got['scores'][b * 4] == -INF and got['tot'][b * 4] == -INF       # the slot lost
        assert got['node_count'][b] == 6 and got['node_uplink'][b, 2] == 0 and got['node_score'][b, 2] == -INF
        assert got['node_uplink'][b, 0] == -1 and got['node_uplink'][b, 1] == -1              # the walk ended at node 0


# ---------------------------------------------------------------- 3. the graph step entry

def _step(entry, c, d, fin_mask=None, tot_out=None):
    cov_on = c['coverage_weight'] > 0
    st = dict(d['state'], new_input=d['new_input'], parent=d['parent'])
    args = (d['logits'], d['att'], d['lens'], d['lm_cost'], c['lm_weight'], d['scores_in'], d['scores_out'],
            d['est_in'], d['est_out'], d['cov_in'] if cov_on else None, d['cov_out'] if cov_on else None,
            d['min_eos'], c['step'], c['B'], c['beam'], c['len_div'], c['min_attention_pos'], c['coverage_tau'],
            c['coverage_weight'], st)
    if entry == 'graph':
        native().beam_lm_step_graph(*(args + (fin_mask, tot_out)))
    else:
        native().beam_lm_step(*args)
    torch.cuda.synchronize()
    return collect(d)


@pytest.mark.parametrize('case', lr.SINGLE_CASES, ids=str)
def test_graph_step_entry_is_the_step_entry_plus_two_outputs(case):
    c = lr.single_case(*case)
    want, margins = lr.lm_beam_step_ref(c)
    tol, _ = lr.tolerance(c, want)
    assert lr.min_margin(margins) > dr.MARGIN_FLOOR
    hyps = c['B'] * c['beam']
    plain = _step('plain', c, buffers(c))
    fin_mask = torch.full((hyps,), lr.POISON, dtype=torch.int32, device=DEV)
    tot_out = torch.full((hyps,), float('nan'), device=DEV)
    graph = _step('graph', c, buffers(c), fin_mask, tot_out)
    for k, v in plain.items():
        if v is None:
            assert graph[k] is None
        else:
            assert v.tobytes() == graph[k].tobytes(), k               # every shared output bit for bit
    assert lr.judge(c, graph, want, tol) == []
    wmask, wtot = gr.step_extras_ref(c, want)
    np.testing.assert_array_equal(fin_mask.cpu().numpy(), wmask)      # (POISON kept for frozen utterances)
    gtot = tot_out.cpu().numpy().astype(np.float64)
    fin = np.isfinite(wtot)
    assert np.array_equal(gtot[~fin], wtot[~fin], equal_nan=True)
    real = fin & (np.abs(wtot) < 1e18)                                # (-lm_weight * 1e20: an exact tie in fp32)
    assert np.abs(gtot[real] - wtot[real]).max(initial=0.0) <= tol
    assert np.array_equal(gtot[fin & ~real], wtot[fin & ~real].astype(np.float32).astype(np.float64))
    if c['step'] == 0:
        assert not wmask[np.repeat(want['live'], c['beam'])].any()


# ---------------------------------------------------------------- 4. step by step

GOLDEN = np.load(os.path.join(lr.GOLDEN, 'beam_lm.npz'))
# utterance 0 is the golden GraphSearch trajectory; seed 221 for the others: scanned on the CPU for
# margins above the floor (smallest 1.6e-3, the golden utterance's own) and for a merge either way
TRAJ = dict(B=3, beam=4, C=7, steps=11, seed=221, lens=[12, 9, 6], T=12, span=2, thr=0.3)


def _traj_inputs():
    tr = TRAJ
    logits, att = gr.traj_inputs(tr['B'], tr['beam'], tr['C'], tr['steps'], tr['seed'], tr['lens'], tr['T'])
    for s in range(tr['steps']):
        logits[s][:tr['beam']] = GOLDEN['logits'][s][0]
        att[s][:tr['beam']] = GOLDEN['att'][s].T
    return logits, att


def _np_store(search):
    return {k: v.cpu().numpy() for k, v in search._store.items()}


def test_device_graph_search_step_by_step_and_finalize():
    from att_speech.modules.beam_search import DeviceGraphSearch, GraphSearch
    tr = TRAJ
    B, beam, C, steps, lens, T = tr['B'], tr['beam'], tr['C'], tr['steps'], tr['lens'], tr['T']
    lm, mapping, p = lr.toy_lm(), lr.TOY_MAPPING, lr.PARAMS
    hash_dec = gr.hash_dec_of(tr['span'])
    logits, att = _traj_inputs()
    search = DeviceGraphSearch(hash_dec, tr['thr'], tr['span'], lm, p['lm_weight'], mapping, p['min_attention_pos'],
                               p['coverage_tau'], p['coverage_weight'], B, beam, torch.device(DEV), C, lr.LN, steps, T,
                               lens, keep_eos_score=False)
    events = gr.collections.Counter()
    for s in range(steps):
        i, o = s & 1, (s + 1) & 1
        st = {k: search._state[k].cpu().numpy() for k in lr.STATE_KEYS}
        bags = lr.arrays_to_bags(*(x.cpu().numpy() for x in search._bags[i]))
        c = dict(logits=logits[s], att=att[s], lens=np.array(lens, np.int32), scores_in=search._scores[i].cpu().numpy(),
                 est_in=search._est[i].cpu().numpy(), cov_in=search._cov[i].cpu().numpy(), min_eos=None, step=s, B=B,
                 beam=beam, C=C, T=T, Lcap=steps + 1, len_div=float(s ** lr.LN) if s > 0 else 1.0, state=st, **p)
        c['lm_cost'] = lr.label_costs_ref(lm, bags, mapping, C)
        before = dict(scores_out=search._scores[o].cpu().numpy(), est_out=search._est[o].cpu().numpy(),
                      cov_out=search._cov[o].cpu().numpy(), new_input=search._state['new_input'].cpu().numpy(),
                      parent=search._state['parent'].cpu().numpy())
        tot_before, mask_before = search._tot.cpu().numpy(), search._fin_mask.cpu().numpy()
        store_before = _np_store(search)
        want, margins = lr.lm_beam_step_ref(c)
        assert lr.min_margin(margins) > dr.MARGIN_FLOOR, (s, margins)
        tol = lr.tolerance(c, want)[0]
        rows = np.repeat(want['live'], beam)
        wmask, wtot = gr.step_extras_ref(c, want)
        new_bags = lr.bag_advance_ref(lm, bags, np.where(rows, want['parent'], 0), np.where(rows, want['new_input'], 0), mapping)
        est_out = before['est_out'].copy()
        est_out[rows, :s + 1] = want['est'][rows]
        mc = dict(att=att[s], lens=np.array(lens, np.int32), scores=np.where(rows, want['scores_out'], before['scores_out']),
                  tot=np.where(rows, wtot, tot_before), est_in=c['est_in'], est_out=est_out,
                  fin_mask=np.where(rows, wmask, mask_before), bags=new_bags, nsteps=want['nsteps'], parent=want['parent'],
                  step=s, B=B, beam=beam, span=tr['span'], merge_threshold=tr['thr'], length_normalization=lr.LN,
                  store=store_before)
        mwant, mm, ev = gr.merge_ref(mc)
        assert gr.min_margin(mm) > dr.MARGIN_FLOOR, (s, mm)
        events.update(ev)
        search.step(t(logits[s], torch.float32), t(att[s], torch.float32))
        torch.cuda.synchronize()
        got = {k: search._state[k].cpu().numpy() for k in lr.STATE_KEYS + ('new_input', 'parent')}
        got.update(scores_out=search._scores[o].cpu().numpy(), est_out=search._est[o].cpu().numpy(),
                   cov_out=search._cov[o].cpu().numpy(), min_eos=None)
        want_after = dict(want, scores_out=np.where(rows, mwant['scores'], want['scores_out']))
        assert lr.judge(c, got, want_after, tol, before=before) == [], s
        np.testing.assert_array_equal(search._fin_mask.cpu().numpy(), mc['fin_mask'])
        mgot = dict(_np_store(search), scores=got['scores_out'], tot=search._tot.cpu().numpy())
        assert gr.judge_merge(mc, mgot, mwant, tol) == [], s
    assert events['old_wins'] > 0 and events['new_wins'] > 0 and events['finished_marks'] > 0 and events['drops'] > 0
    search.finalize()
    assert search.overflow == 0
    graphs = search.get_graph()
    merged = marks = dead = 0
    for b in range(B):
        host = GraphSearch(hash_dec, tr['thr'], lm, p['lm_weight'], mapping, p['min_attention_pos'], p['coverage_tau'],
                           p['coverage_weight'], 1, beam, torch.device('cpu'), C, lr.LN, keep_eos_score=False)
        sl = slice(b * beam, (b + 1) * beam)
        for s in range(steps):
            host.step(torch.from_numpy(logits[s][sl])[None].clone(), att_weights=torch.from_numpy(att[s][sl, :lens[b]].T.copy()))
            if host.has_finished():
                break
        dead += int((~np.isfinite(host.scores.numpy())).sum())
        V, Vs, E = gr.graph_arrays(graphs[b])
        hV, hVs, hE = gr.graph_arrays(host.get_graph()[0])
        np.testing.assert_array_equal(V, hV)
        np.testing.assert_array_equal(E, hE)
        np.testing.assert_allclose(Vs, hVs, rtol=1e-5, atol=1e-5)
        merged += int(E[:, 2].sum())
        marks += int(V[:, 2].sum())
        alive = np.isfinite(host.scores.numpy())
        assert np.array_equal(np.isfinite(search.scores[b].numpy()), alive)
        np.testing.assert_array_equal(search.estimations[b].numpy()[alive], host.estimations.numpy()[alive])
    assert merged > 0 and marks > 0 and dead > 0                      # not vacuous


@pytest.mark.parametrize('beam,span,seed', [(3, 2, 4), (4, 1, 21)])
def test_search_without_an_lm_term_equals_the_host_class(beam, span, seed):
    """lm_weight == 0 with coverage on: no bags, no LM-state test, nodes carry an empty set.  The
    trajectories of tests/test_graph_search_referee.py (margins asserted there on the same inputs)."""
    from att_speech.modules.beam_search import DeviceGraphSearch, GraphSearch
    C, T, steps, thr, p = 7, 12, 10, 0.5, lr.PARAMS
    logits, att = gr.traj_inputs(1, beam, C, steps, seed, [T], T)
    args = (lr.toy_lm(), 0.0, lr.TOY_MAPPING, p['min_attention_pos'], p['coverage_tau'], p['coverage_weight'], 1, beam)
    host = GraphSearch(gr.hash_dec_of(span), thr, *args, torch.device('cpu'), C, lr.LN, keep_eos_score=False)
    search = DeviceGraphSearch(gr.hash_dec_of(span), thr, span, *args, torch.device(DEV), C, lr.LN, steps, T, [T])
    for s in range(steps):
        host.step(torch.from_numpy(logits[s])[None].clone(), att_weights=torch.from_numpy(att[s].T.copy()))
        search.step(t(logits[s], torch.float32), t(att[s], torch.float32))
        assert search.poll_finished() == host.has_finished()
        if host.has_finished():
            break
    search.finalize()
    V, Vs, E = gr.graph_arrays(search.get_graph()[0])
    hV, hVs, hE = gr.graph_arrays(host.get_graph()[0])
    np.testing.assert_array_equal(V, hV)
    np.testing.assert_array_equal(E, hE)
    np.testing.assert_allclose(Vs, hVs, rtol=1e-5, atol=1e-5)
    assert int(E[:, 2].sum()) > 0 and all(n[2][0] == set() for li in search.graph[0].values() for n in li)
    np.testing.assert_allclose(search.scores[0].numpy(), host.scores.numpy(), rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- 5. end to end

VOCAB = ['<pad>', '<unk>', ' ', 'a', 'b', 'c']
# model seed 1, merge key of 2 labels, threshold 0.8: picked on the CPU (host decode per utterance,
# replayed through gr.RefGraphSearch) for 6 merged edges per utterance and a smallest margin of 0.011
E2E = dict(seed=1, span=2, thr=0.8)


def _decoder(lm):
    from att_speech.modules.tcn import AttentionDecoderTCN
    torch.manual_seed(E2E['seed'])
    dec = AttentionDecoderTCN({'features': torch.zeros(14, 3, 16)}, 6, tcn_hidden_size=32, att_hidden_size=8,
                              dropout_p=0.0, kernel_size=3, dilation_sizes=[1, 2], beam_size=3, length_normalization=0.6,
                              vocabulary=VOCAB, lm_file=lm, lm_weight=0.5, coverage_weight=0.1, coverage_tau=0.1,
                              min_attention_pos=0.3, use_graph_search=True, graph_search_history_len=E2E['span'],
                              graph_search_merge_threshold=E2E['thr']).eval().to(DEV)
    dec.TRANSCRIPTION_LEN_GUARD = 12
    return dec


def test_decode_of_a_batch_is_the_host_graph_search_of_each_utterance(monkeypatch):
    from att_speech.modules.beam_search import DeviceGraphSearch, GraphSearch
    for name in ('ASR_TCN_NATIVE', 'ASR_TCN_FF_NATIVE', 'ASR_LM_BEAM_NATIVE', 'ASR_GRAPH_SEARCH_NATIVE'):
        monkeypatch.delenv(name, raising=False)
    dec = _decoder(lr.toy_lm())
    lens, B, beam, C, T = [14, 9, 6], 3, 3, 7, 14
    enc = torch.randn(14, 3, 16, generator=torch.Generator().manual_seed(5))
    for b, ln in enumerate(lens):
        enc[ln:, b] = 0
    enc = enc.to(DEV)
    # the switch unset: a single utterance runs the host class, a batch is the reference's assert
    hosts = []
    with torch.no_grad():
        for b in range(B):
            hosts.append(dec.decode(enc[:lens[b], b:b + 1].contiguous(), torch.tensor([lens[b]])))
        with pytest.raises(AssertionError):
            dec.decode(enc, torch.tensor(lens))
    assert all(type(h['beam_search']) is GraphSearch for h in hosts)
    assert max(sum(e[2] == 'merged' for e in h['graph'][0]['E']) for h in hosts) > 0
    monkeypatch.setenv('ASR_GRAPH_SEARCH_NATIVE', '1')
    with torch.no_grad():
        res = dec.decode(enc, torch.tensor(lens))
        traced = dec.decode(enc, torch.tensor(lens), return_attention=True)
        one = dec.decode(enc[:lens[1], 1:2].contiguous(), torch.tensor([lens[1]]))
    assert isinstance(res['beam_search'], DeviceGraphSearch) and isinstance(one['beam_search'], DeviceGraphSearch)
    # every decision of the trajectory is clear: the referee replays the device's own logits / alignments
    rs = gr.RefGraphSearch(E2E['span'], E2E['thr'], lr.toy_lm(), dec.alphabet_mapping, B, beam, C, T, lens,
                           dec.TRANSCRIPTION_LEN_GUARD + 1, keep_eos=False, lm_weight=0.5, coverage_weight=0.1,
                           coverage_tau=0.1, min_attention_pos=0.3)
    assert len(traced['logits']) >= 1 and len(traced['attweights']) == len(traced['logits']) + 1
    for lg, at in zip(traced['logits'], traced['attweights'][1:]):
        rs.step(lg[0].double().cpu().numpy(), np.ascontiguousarray(at.t().double().cpu().numpy()))
    worst = min([lr.min_margin(m) for m in rs.margins] + [gr.min_margin(m) for m in rs.merge_margins])
    print('smallest margin over %d steps: %.3g; events %s' % (len(rs.margins), worst, dict(rs.events)))
    assert worst > dr.MARGIN_FLOOR and rs.events['old_wins'] + rs.events['new_wins'] > 0
    assert len(res['graph']) == B and len(one['graph']) == 1
    for b, h in enumerate(hosts):
        assert [int(v) for v in res['decoded'][b]] == [int(v) for v in h['decoded'][0]], b
        for k, v in h['decoded_scores'].items():
            np.testing.assert_allclose(res['decoded_scores'][k][b], v[0], rtol=1e-4, atol=1e-6)
        for G in (res['graph'][b], traced['graph'][b]) + ((one['graph'][0],) if b == 1 else ()):
            V, Vs, E = gr.graph_arrays(G)
            hV, hVs, hE = gr.graph_arrays(h['graph'][0])
            np.testing.assert_array_equal(V, hV)
            np.testing.assert_array_equal(E, hE)
            np.testing.assert_allclose(Vs, hVs, rtol=1e-4, atol=1e-5)
        hs = h['beam_search']
        alive = np.isfinite(hs.scores.cpu().numpy())
        assert np.array_equal(np.isfinite(res['beam_search'].scores[b].numpy()), alive)
        np.testing.assert_array_equal(res['beam_search'].estimations[b].numpy()[alive], hs.estimations.cpu().numpy()[alive])
        np.testing.assert_allclose(res['beam_search'].scores[b].numpy()[alive], hs.scores.cpu().numpy()[alive],
                                   rtol=1e-4, atol=1e-5)
    # ASR_LM_BEAM_NATIVE=0 still sends it to the host
    monkeypatch.setenv('ASR_LM_BEAM_NATIVE', '0')
    with torch.no_grad():
        back = dec.decode(enc[:lens[1], 1:2].contiguous(), torch.tensor([lens[1]]))
    assert type(back['beam_search']) is GraphSearch


def test_store_above_the_budget_falls_back_to_the_host(monkeypatch):
    import warnings
    from att_speech import _native
    from att_speech.modules import beam_search as bs
    for name in ('ASR_TCN_NATIVE', 'ASR_TCN_FF_NATIVE', 'ASR_LM_BEAM_NATIVE'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('ASR_GRAPH_SEARCH_NATIVE', '1')
    monkeypatch.setattr(bs, 'GRAPH_STORE_BUDGET_BYTES', 1000)
    _native._WARNED.pop('graph_store', None)
    dec = _decoder(lr.toy_lm())
    enc = torch.randn(14, 2, 16, generator=torch.Generator().manual_seed(6)).to(DEV)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        with torch.no_grad():
            both = dec.decode(enc, torch.tensor([14, 14]))
            dec.decode(enc, torch.tensor([14, 14]))
    assert len([r for r in rec if 'node store' in str(r.message)]) == 1       # warned once
    assert all(type(s) is bs.GraphSearch for s in both['beam_search'])
    assert len(both['graph']) == 2 and all(set(g) == {'V', 'E'} for g in both['graph'])


# ---------------------------------------------------------------- 6. argument checks

def test_argument_checks_launch_nothing():
    c = gr.merge_cases()['span2']

    def refused(exc, mutate):
        d = merge_buffers(c)
        whole = dict(d)
        kw = mutate(d) or {}
        with pytest.raises(exc):
            merge_launch(c, d, **kw)
        torch.cuda.synchronize()
        for k in gr.NODE_KEYS:
            assert np.array_equal(whole[k].cpu().numpy(), c['store'][k], equal_nan=True), k
        assert np.array_equal(whole['scores'].cpu().numpy(), c['scores']) and np.array_equal(whole['tot'].cpu().numpy(), c['tot'])

    refused(NotImplementedError, lambda d: dict(beam=33, B=1))
    refused(AssertionError, lambda d: dict(step=c['est_in'].shape[1]))                          # Lcap == step
    refused(AssertionError, lambda d: dict(span=-1))
    refused(AssertionError, lambda d: d.update(tot=None))
    refused(AssertionError, lambda d: d.update(node_uplink=None))
    refused(AssertionError, lambda d: d.update({k: d[k][:, :8].contiguous() for k in gr.NODE_KEYS[1:]}))   # Ncap 8 < 4 * 4
    refused(NotImplementedError, lambda d: d.update(att=torch.zeros(12, 8161, device=DEV)))
    # the graph step entry without its two outputs
    sc = lr.single_case(3, 3, 6, 1, 'toy')
    d = buffers(sc)
    with pytest.raises(AssertionError):
        _step('graph', sc, d, None, torch.zeros(9, device=DEV))
    with pytest.raises(AssertionError):
        _step('graph', sc, d, torch.zeros(9, dtype=torch.int32, device=DEV), None)
    torch.cuda.synchronize()
    g, pre = collect(d), lr.prefilled(sc)
    for k in ('est_out', 'new_input', 'parent'):
        assert np.array_equal(g[k], pre[k]), k
    assert np.isnan(g['scores_out']).all()
    assert native().graph_search_supported(32, 0, 8160) and not native().graph_search_supported(33, 0, 12)
