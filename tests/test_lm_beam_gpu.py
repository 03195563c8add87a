"""The device LM-fused beam search (asr_lm_label_costs_f64, asr_beam_lm_step_f32,
asr_lm_bag_advance_f64, DeviceBeamSearchLM, AttentionDecoderTCN.decode with lm_file) against the
fp64 referees of tests/lm_beam_referee.py, proved on the CPU by tests/test_lm_beam_referee.py.

Integer outputs are bit-equal to the referee; every case is seeded so that each live decision has
a margin above decode_referee.MARGIN_FLOOR (asserted), or is an exact tie.  fp32 scores are held
to 4x the distance of the referee's own fp32 run from its fp64 run plus 4 fp32 ulps of the largest
operand (the same rule, for the same reason, as tests/test_decode_step_gpu.py: the kernel's
log-softmax sums in another order than torch's, each within a few ulps of the fp64 value, so a small
multiple of the fp32 evaluation's own distance bounds it; the ulp term covers scores that the fp32
run happens to hit exactly).  LM costs (fp64) to 1e-9 relative."""
import os
import warnings

import numpy as np
import pytest
import torch

import decode_referee as dr
import lm_beam_referee as lr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F_STATE = ('fin_score', 'best_score', 'best_elems')


def native():
    from att_speech import _native
    return _native


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


def buffers(c):
    pre = lr.prefilled(c)
    d = {k: t(v) for k, v in pre.items()}
    d['state'] = {k: t(v, torch.float32 if k in F_STATE else torch.int32) for k, v in c['state'].items()}
    d.update(logits=t(c['logits'], torch.float32), att=t(c['att'], torch.float32), lens=t(c['lens']),
             scores_in=t(c['scores_in'], torch.float32), est_in=t(c['est_in']),
             cov_in=None if c['cov_in'] is None else t(c['cov_in'], torch.float32),
             min_eos=None if c['min_eos'] is None else t(c['min_eos'], torch.float32),
             lm_cost=None if c['lm_cost'] is None else t(c['lm_cost']))
    return d


def launch(c, d, **kw):
    a = dict(c, **kw)
    cov_on = a['coverage_weight'] > 0
    st = dict(d['state'], new_input=d['new_input'], parent=d['parent'], fin_parity=d['state']['fin_parity'])
    native().beam_lm_step(d['logits'], d['att'], d['lens'], d['lm_cost'], a['lm_weight'], d['scores_in'],
                          d['scores_out'], d['est_in'], d['est_out'], d['cov_in'] if cov_on else None,
                          d['cov_out'] if cov_on else None, d['min_eos'], a['step'], a['B'], a['beam'],
                          a['len_div'], a['min_attention_pos'], a['coverage_tau'], a['coverage_weight'], st)
    torch.cuda.synchronize()
    return collect(d)


def collect(d):
    got = {k: v.cpu().numpy() for k, v in d['state'].items()}
    got.update({k: d[k].cpu().numpy() for k in ('scores_out', 'est_out', 'cov_out', 'new_input', 'parent')})
    got['min_eos'] = None if d['min_eos'] is None else d['min_eos'].cpu().numpy()
    return got


# ---------------------------------------------------------------- 1. one launch from arbitrary state

@pytest.mark.parametrize('case', lr.SINGLE_CASES, ids=str)
def test_step_from_arbitrary_state(case):
    c = lr.single_case(*case)
    want, margins = lr.lm_beam_step_ref(c)
    tol, d32 = lr.tolerance(c, want)
    assert lr.min_margin(margins) > dr.MARGIN_FLOOR and 10 * tol <= dr.MARGIN_FLOOR
    # the label costs first, from the bags, into a POISON-ed buffer
    lm = c['lm'].device_arrays(torch.device(DEV))
    bs, bw, bn = (t(x) for x in lr.bags_to_arrays(c['bags']))
    cost = torch.full((c['B'] * c['beam'], c['C']), float('nan'), dtype=torch.float64, device=DEV)
    native().lm_label_costs(lm, bs, bw, bn, t(np.array(c['mapping'], np.int32)), t(c['state']['frozen']),
                            c['B'], c['beam'], c['C'], cost)
    cost = cost.cpu().numpy()
    rows = np.repeat(c['state']['frozen'] == 0, c['beam'])
    assert np.isnan(cost[~rows]).all()
    fin = np.isfinite(c['lm_cost'][rows])
    assert np.array_equal(np.isfinite(cost[rows]), fin) and np.array_equal(cost[rows][~fin], c['lm_cost'][rows][~fin])
    rel = np.abs(cost[rows][fin] - c['lm_cost'][rows][fin]) / np.abs(c['lm_cost'][rows][fin])
    assert rel.max(initial=0.0) <= 1e-9
    # the step, fed with the referee's costs
    d = buffers(c)
    got = launch(c, d)
    print('%s smallest margin %.3g  fp32 distance %.3g  tolerance %.3g  LM cost error %.3g' % (
        case, lr.min_margin(margins), d32, tol, rel.max(initial=0.0)))
    assert lr.judge(c, got, want, tol) == []
    # the survivors' bags
    out = [torch.full_like(bs, lr.POISON), torch.full_like(bw, float('nan')), torch.full_like(bn, lr.POISON)]
    over = torch.zeros(1, dtype=torch.int32, device=DEV)
    native().lm_bag_advance(lm, t(np.array(c['mapping'], np.int32)), (bs, bw, bn), out, d['parent'], d['new_input'],
                            d['state']['nsteps'], c['step'], c['B'], c['beam'], over)
    torch.cuda.synchronize()
    live = np.repeat(want['live'], c['beam'])
    wb = lr.bag_advance_ref(c['lm'], c['bags'], np.where(live, want['parent'], 0), np.where(live, want['new_input'], 0),
                            c['mapping'])
    ws, ww, wn = lr.bags_to_arrays([wb[h] if live[h] else {} for h in range(len(live))])
    gs, gw, gn = (x.cpu().numpy() for x in out)
    assert int(over) == 0
    assert np.array_equal(gn[live], wn[live]) and (gn[~live] == lr.POISON).all()
    assert np.array_equal(gs[live], ws[live]) and (gs[~live] == lr.POISON).all()      # POISON beyond n too
    f = np.isfinite(ww)
    assert np.isnan(gw[~f]).all()                                                     # NaN beyond n and in frozen rows
    np.testing.assert_allclose(gw[f], ww[f], rtol=1e-9)


# ---------------------------------------------------------------- 2. exact ties

def test_exact_ties():
    cases = lr.tie_cases()
    for name in ('lowest_flat_index_wins', 'all_equal_everywhere', 'first_step_equal'):
        c = cases[name]
        want, _ = lr.lm_beam_step_ref(c)
        assert lr.judge(c, launch(c, buffers(c)), want, lr.tolerance(c, want)[0]) == [], name
    c1 = cases['finish_beam_0']
    d1 = buffers(c1)
    g1 = launch(c1, d1)
    assert g1['fin_count'].tolist() == [1] and g1['best_len'].tolist() == [1]
    c2 = lr.tie_second_launch(c1, {k: g1[k] for k in lr.STATE_KEYS})
    g2 = launch(c2, buffers(c2))
    p = g2['fin_parity'][0]
    assert g2['fin_count'].tolist() == [2]
    assert g2['fin_score'][p, 0, 0].tobytes() == g2['fin_score'][p, 0, 1].tobytes()     # an exact tie
    assert g2['fin_beam'][p, 0, :2].tolist() == [0, 1]                                  # older first
    assert g2['best_score'].tobytes() == g1['best_score'].tobytes()                     # equal does not replace
    assert g2['best_tokens'][0, 0] == c1['est_in'][0, 0] and g2['best_len'].tolist() == [1]
    assert g2['best_elems'].tobytes() == g1['best_elems'].tobytes()


# ---------------------------------------------------------------- 3. step by step

def _search(lm, mapping, B, beam, C, lens, steps, keep_eos=True, **params):
    from att_speech.modules.beam_search import DeviceBeamSearchLM
    p = dict(lr.PARAMS, **params)
    return DeviceBeamSearchLM(lm, p['lm_weight'], mapping, p['min_attention_pos'], p['coverage_tau'],
                              p['coverage_weight'], B, beam, torch.device(DEV), C, lr.LN, steps, lr.T_FRAMES,
                              lens, keep_eos_score=keep_eos)


def _snapshot(s):
    ts = s._scores + s._est + s._cov + [s._min_eos, s._cost] + list(s._bags[0]) + list(s._bags[1]) + \
        [v for k, v in s._state.items()]
    return [x.clone() for x in ts if x is not None]


def _utterance_bytes(s, b):
    beam = s.beam_size
    out = []
    for x in s._scores + s._est + s._cov + [s._min_eos, s._cost] + list(s._bags[0]) + list(s._bags[1]):
        out.append(x[b * beam:(b + 1) * beam].cpu().numpy().tobytes())
    for k, v in s._state.items():
        if k in ('fin_score', 'fin_len', 'fin_beam', 'fin_tokens'):
            out.append(v[:, b].cpu().numpy().tobytes())
        elif k in ('new_input', 'parent'):
            out.append(v[b * beam:(b + 1) * beam].cpu().numpy().tobytes())
        elif k not in ('flags', 'overflow'):
            out.append(v[b].cpu().numpy().tobytes())
    return out


def test_device_search_step_by_step_and_finalize():
    from att_speech.modules.beam_search import BeamSearchLM
    tr = lr.TRAJ
    B, beam, C, steps, lens = tr['B'], tr['beam'], tr['C'], tr['steps'], tr['lens']
    lm, mapping = lr.toy_lm(), lr.TOY_MAPPING
    logits, att = lr.traj_inputs(**tr)
    search = _search(lm, mapping, B, beam, C, lens, steps)
    froze_at = {}
    for s in range(steps):
        i, o = s & 1, (s + 1) & 1
        st = {k: search._state[k].cpu().numpy() for k in lr.STATE_KEYS}
        bags = lr.arrays_to_bags(*(x.cpu().numpy() for x in search._bags[i]))
        c = dict(logits=logits[s], att=att[s], lens=np.array(lens, np.int32), scores_in=search._scores[i].cpu().numpy(),
                 est_in=search._est[i].cpu().numpy(), cov_in=search._cov[i].cpu().numpy(),
                 min_eos=search._min_eos.cpu().numpy(), step=s, B=B, beam=beam, C=C, T=lr.T_FRAMES, Lcap=steps + 1,
                 len_div=float(s ** lr.LN) if s > 0 else 1.0, state=st, **lr.PARAMS)
        c['lm_cost'] = lr.label_costs_ref(lm, bags, mapping, C)
        before = dict(scores_out=search._scores[o].cpu().numpy(), est_out=search._est[o].cpu().numpy(),
                      cov_out=search._cov[o].cpu().numpy(), new_input=search._state['new_input'].cpu().numpy(),
                      parent=search._state['parent'].cpu().numpy())
        frozen_bytes = {b: _utterance_bytes(search, b) for b in range(B) if st['frozen'][b]}
        all_bytes = [x.cpu().numpy().tobytes() for x in _snapshot(search)] if st['frozen'].all() else None
        want, margins = lr.lm_beam_step_ref(c)
        assert lr.min_margin(margins) > dr.MARGIN_FLOOR, (s, margins)
        search.step(t(logits[s], torch.float32), t(att[s], torch.float32))
        torch.cuda.synchronize()
        got = {k: search._state[k].cpu().numpy() for k in lr.STATE_KEYS + ('new_input', 'parent')}
        got.update(scores_out=search._scores[o].cpu().numpy(), est_out=search._est[o].cpu().numpy(),
                   cov_out=search._cov[o].cpu().numpy(), min_eos=search._min_eos.cpu().numpy())
        assert lr.judge(c, got, want, lr.tolerance(c, want)[0], before=before) == [], s
        # the label costs the device used, and the bags it left
        live = np.repeat(want['live'], beam)
        dc = search._cost.cpu().numpy()[live]
        f = np.isfinite(c['lm_cost'][live])
        assert np.array_equal(np.isfinite(dc), f)
        np.testing.assert_allclose(dc[f], c['lm_cost'][live][f], rtol=1e-9)
        wb = lr.bag_advance_ref(lm, bags, np.where(live, want['parent'], 0), np.where(live, want['new_input'], 0), mapping)
        gb = lr.arrays_to_bags(*(x.cpu().numpy() for x in search._bags[o]))
        for h in np.nonzero(live)[0]:
            assert list(gb[h]) == list(wb[h])
            np.testing.assert_allclose(list(gb[h].values()), list(wb[h].values()), rtol=1e-9)
        # launches change nothing of a frozen utterance, and nothing at all once all are
        for b, old in frozen_bytes.items():
            assert _utterance_bytes(search, b) == old, (s, b)
        if all_bytes is not None:
            assert [x.cpu().numpy().tobytes() for x in _snapshot(search)] == all_bytes
        for b in range(B):
            if got['frozen'][b] and b not in froze_at:
                froze_at[b] = s + 1
        assert search.poll_finished() == bool(got['frozen'].all())
    assert sorted(froze_at) == [0, 1, 2] and froze_at[2] < froze_at[0]        # one froze early
    search.finalize()
    assert search.overflow == 0
    for b in range(B):
        host = BeamSearchLM(lm, lr.PARAMS['lm_weight'], mapping, lr.PARAMS['min_attention_pos'],
                            lr.PARAMS['coverage_tau'], lr.PARAMS['coverage_weight'], 1, beam, torch.device('cpu'), C,
                            lr.LN, keep_eos_score=True)
        sl = slice(b * beam, (b + 1) * beam)
        for s in range(steps):
            host.step(torch.from_numpy(logits[s][sl])[None].clone(),
                      att_weights=torch.from_numpy(att[s][sl, :lens[b]].T.copy()))
            if host.has_finished():
                break
        assert s + 1 == froze_at[b]
        assert search.best_finished[b].tolist() == host.best_finished[0].tolist()
        np.testing.assert_allclose(search.best_finished_scores[b], float(host.best_finished_scores[0]), rtol=1e-5)
        for k, v in host.best_finished_scores_elements.items():
            np.testing.assert_allclose(search.best_finished_scores_elements[k][b], v[0], rtol=1e-5, atol=1e-6)
        assert len(search.finished[b]) == len(host.finished)
        for mine, theirs in zip(search.finished[b], host.finished):
            np.testing.assert_allclose(float(mine[0]), float(theirs[0]), rtol=1e-5)
            assert mine[1].tolist() == theirs[1].tolist() and mine[2] == theirs[2]
        alive = np.isfinite(host.scores.numpy())
        assert np.array_equal(np.isfinite(search.scores[b].numpy()), alive)
        np.testing.assert_array_equal(search.estimations[b].numpy()[alive], host.estimations.numpy()[alive])
        np.testing.assert_allclose(search.scores[b].numpy()[alive], host.scores.numpy()[alive], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(search.coverage[b].numpy()[:, alive], host.coverage.numpy()[:, alive], rtol=1e-5, atol=1e-6)
        for k in np.nonzero(alive)[0]:
            assert sorted(search.fst_states[b][k]) == sorted(host.fst_states[k])
            np.testing.assert_allclose([search.fst_states[b][k][q] for q in sorted(host.fst_states[k])],
                                       [host.fst_states[k][q] for q in sorted(host.fst_states[k])], rtol=1e-9)


# ---------------------------------------------------------------- 4. end to end

VOCAB = ['<pad>', '<unk>', ' ', 'a', 'b', 'c']


def _decoder(lm, seed=0, **kw):
    from att_speech.modules.tcn import AttentionDecoderTCN
    torch.manual_seed(seed)
    args = dict(tcn_hidden_size=32, att_hidden_size=8, dropout_p=0.0, kernel_size=3, dilation_sizes=[1, 2],
                beam_size=3, length_normalization=0.6, vocabulary=VOCAB, lm_file=lm, lm_weight=0.5,
                coverage_weight=0.1, coverage_tau=0.1, min_attention_pos=0.3)
    args.update(kw)
    dec = AttentionDecoderTCN({'features': torch.zeros(14, 3, 16)}, 6, **args).eval().to(DEV)
    dec.TRANSCRIPTION_LEN_GUARD = 12
    return dec


def _host_decode(dec, enc, lens):
    old = os.environ.get('ASR_LM_BEAM_NATIVE')
    os.environ['ASR_LM_BEAM_NATIVE'] = '0'
    try:
        with torch.no_grad():
            return [dec.decode(enc[:lens[b], b:b + 1].contiguous(), torch.tensor([lens[b]])) for b in range(len(lens))]
    finally:
        if old is None:
            del os.environ['ASR_LM_BEAM_NATIVE']
        else:
            os.environ['ASR_LM_BEAM_NATIVE'] = old


def test_decode_of_a_batch_is_the_host_decode_of_each_utterance():
    from att_speech.modules.beam_search import BeamSearchLM, DeviceBeamSearchLM
    # model seed 4 and these lengths: picked on the CPU (host decode per utterance, replayed through
    # lr.RefSearch) for a smallest margin of 0.011 along the whole trajectory; asserted below on the
    # device's own logits and alignments.  (A length of 10 would put the uniform initial alignment
    # of 1/10 exactly on coverage_tau.)  With random weights no hypothesis finishes in the 12 steps,
    # so the final beams are compared too.
    dec = _decoder(lr.toy_lm(), seed=4)
    gen = torch.Generator().manual_seed(5)
    lens = [14, 9, 6]
    B, beam, C, T = 3, 3, 7, 14
    enc = torch.randn(14, 3, 16, generator=gen)
    for b, ln in enumerate(lens):
        enc[ln:, b] = 0
    enc = enc.to(DEV)
    with torch.no_grad():
        res = dec.decode(enc, torch.tensor(lens))
        traced = dec.decode(enc, torch.tensor(lens), return_attention=True)
    assert isinstance(res['beam_search'], DeviceBeamSearchLM)
    # every decision of the trajectory is clear: the referee replays the device's logits / alignments
    rs = lr.RefSearch(lr.toy_lm(), dec.alphabet_mapping, B, beam, C, T, lens, dec.TRANSCRIPTION_LEN_GUARD + 1,
                      keep_eos=False, lm_weight=0.5, coverage_weight=0.1, coverage_tau=0.1, min_attention_pos=0.3)
    assert len(traced['logits']) >= 1 and len(traced['attweights']) == len(traced['logits']) + 1
    for lg, at in zip(traced['logits'], traced['attweights'][1:]):
        rs.step(lg[0].double().cpu().numpy(), np.ascontiguousarray(at.t().double().cpu().numpy()))
    worst = min(lr.min_margin(m) for m in rs.margins)
    print('smallest margin over %d steps: %.3g' % (len(rs.margins), worst))
    assert worst > dr.MARGIN_FLOOR
    for b in range(B):
        n = int(rs.state['nsteps'][b])
        alive = np.isfinite(rs.scores[b * beam:(b + 1) * beam])
        np.testing.assert_array_equal(traced['beam_search'].estimations[b].numpy()[alive],
                                      rs.est[b * beam:(b + 1) * beam, :n][alive])
        assert [int(v) for v in traced['decoded'][b]] == [int(v) for v in res['decoded'][b]]
    hosts = _host_decode(dec, enc, lens)
    assert all(isinstance(h['beam_search'], BeamSearchLM) for h in hosts)
    assert set(res['decoded_scores']) == set(hosts[0]['decoded_scores']) == {'acoustic', 'lm', 'coverage'}
    for b, h in enumerate(hosts):
        assert [int(v) for v in res['decoded'][b]] == [int(v) for v in h['decoded'][0]], b
        for k, v in h['decoded_scores'].items():
            np.testing.assert_allclose(res['decoded_scores'][k][b], v[0], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(res['beam_search'].best_finished_scores[b],
                                   float(h['beam_search'].best_finished_scores[0]), rtol=1e-4)
        hs = h['beam_search']
        alive = np.isfinite(hs.scores.cpu().numpy())
        assert np.array_equal(np.isfinite(res['beam_search'].scores[b].numpy()), alive)
        np.testing.assert_array_equal(res['beam_search'].estimations[b].numpy()[alive],
                                      hs.estimations.cpu().numpy()[alive])
        np.testing.assert_allclose(res['beam_search'].scores[b].numpy()[alive], hs.scores.cpu().numpy()[alive],
                                   rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(res['loss']), np.mean([float(h['loss']) for h in hosts]), rtol=1e-4)
    # the host path with the whole batch is the reference's assert
    os.environ['ASR_LM_BEAM_NATIVE'] = '0'
    try:
        with pytest.raises(AssertionError):
            dec.decode(enc, torch.tensor(lens))
    finally:
        del os.environ['ASR_LM_BEAM_NATIVE']


# ---------------------------------------------------------------- 5. overflow

def test_bag_overflow_raises_the_flag_and_decode_falls_back():
    from att_speech import _native
    from att_speech.lm_fst import LmFst, SymbolTable
    from att_speech.modules.beam_search import BeamSearchLM
    syms = SymbolTable([(0, '<eps>'), (1, '<spc>'), (2, 'a'), (3, 'b'), (4, 'c')])
    n = 33
    # state 0: 33 arcs of every label to distinct states, each of which loops back on every label
    src = [0] * (4 * n) + [s for s in range(1, n + 1) for _ in range(4)]
    dst = [1 + i for _ in range(4) for i in range(n)] + [0] * (4 * n)
    il = [l for l in (1, 2, 3, 4) for _ in range(n)] + [1, 2, 3, 4] * n
    w = list(np.linspace(0.5, 2.0, len(src)))
    lm = LmFst(n + 1, 0, src, dst, il, il, w, np.zeros(n + 1), syms, syms)
    dec = _decoder(lm, beam_size=2)
    enc = torch.randn(14, 1, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    _native._WARNED.pop('lm_bag_overflow', None)
    os.environ['ASR_LM_BEAM_NATIVE'] = '1'                        # a single utterance: the device search on request
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            with torch.no_grad():
                res = dec.decode(enc, torch.tensor([14]))
                again = dec.decode(enc, torch.tensor([14]))
                # a batch falls back utterance by utterance
                both = dec.decode(torch.cat((enc, enc), 1), torch.tensor([14, 14]))
    finally:
        del os.environ['ASR_LM_BEAM_NATIVE']
    msgs = [str(r.message) for r in rec if 'LM bag' in str(r.message)]
    assert len(msgs) == 1 and '33' in msgs[0]                     # warned once, with the size
    assert isinstance(res['beam_search'], BeamSearchLM) and isinstance(again['beam_search'], BeamSearchLM)
    host = _host_decode(dec, enc, [14])[0]
    assert [int(v) for v in res['decoded'][0]] == [int(v) for v in host['decoded'][0]]
    assert res['decoded_scores'] == host['decoded_scores']
    assert [[int(v) for v in d] for d in both['decoded']] == [[int(v) for v in host['decoded'][0]]] * 2
    assert both['decoded_scores'] == {k: v * 2 for k, v in host['decoded_scores'].items()}
    assert all(isinstance(s, BeamSearchLM) for s in both['beam_search'])
    # unset, a single utterance stays with the host class and raises no flag
    with torch.no_grad():
        assert isinstance(dec.decode(enc, torch.tensor([14]))['beam_search'], BeamSearchLM)


# ---------------------------------------------------------------- 6. argument checks

def test_argument_checks_launch_nothing():
    c = lr.single_case(3, 3, 6, 1, 'toy')

    def refused(exc, mutate):
        d = buffers(c)
        whole = dict(d)                         # (a mutation may take a buffer away; all are checked)
        kw = mutate(d) or {}
        with pytest.raises(exc):
            launch(c, d, **kw)
        torch.cuda.synchronize()
        g = collect(whole)
        pre = lr.prefilled(c)
        for k in ('est_out', 'new_input', 'parent'):
            assert np.array_equal(g[k], pre[k]), k
        assert np.isnan(g['scores_out']).all() and np.isnan(g['cov_out']).all()
        for k in lr.STATE_KEYS:
            assert np.array_equal(g[k], np.asarray(c['state'][k]).astype(g[k].dtype), equal_nan=True), k

    refused(NotImplementedError, lambda d: dict(beam=33, B=1))
    refused(NotImplementedError, lambda d: d.update(logits=torch.zeros(9, 2050, device=DEV)))   # beam * (C-1) = 6147
    refused(AssertionError, lambda d: d.update(scores_out=None))
    refused(AssertionError, lambda d: dict(step=lr.SINGLE_LCAP))                                # Lcap == step
    refused(AssertionError, lambda d: d.update(cov_in=None))                                    # coverage on, no buffer
    # the LM launches: a cap mismatch and null pointers
    lm = c['lm'].device_arrays(torch.device(DEV))
    bs, bw, bn = (t(x) for x in lr.bags_to_arrays(c['bags']))
    mp = t(np.array(c['mapping'], np.int32))
    cost = torch.full((9, c['C']), float('nan'), dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError):
        native().lm_label_costs(lm, bs, bw, bn, mp, None, 3, 3, c['C'], cost, bag_cap=16)
    with pytest.raises(AssertionError):
        native().lm_label_costs(lm, bs, None, bn, mp, None, 3, 3, c['C'], cost)
    out = [torch.full_like(bs, lr.POISON), torch.full_like(bw, float('nan')), torch.full_like(bn, lr.POISON)]
    over = torch.zeros(1, dtype=torch.int32, device=DEV)
    z = torch.zeros(9, dtype=torch.int32, device=DEV)
    ns = torch.full((3,), 2, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError):
        native().lm_bag_advance(lm, mp, (bs, bw, bn), out, z, z, ns, 1, 3, 3, over, bag_cap=64)
    with pytest.raises(AssertionError):
        native().lm_bag_advance(lm, mp, (bs, bw, bn), (bs, out[1], out[2]), z, z, ns, 1, 3, 3, over)   # in place
    with pytest.raises(AssertionError):
        native().lm_bag_advance(lm, mp, (bs, bw, bn), out, z, z, ns, 1, 3, 3, None)
    torch.cuda.synchronize()
    assert torch.isnan(cost).all() and int(over) == 0
    assert bool((out[0] == lr.POISON).all()) and bool(torch.isnan(out[1]).all()) and bool((out[2] == lr.POISON).all())
    assert not native().beam_lm_supported(33, 6) and not native().beam_lm_supported(3, 6, 16)
    assert native().beam_lm_supported(32, 65)
