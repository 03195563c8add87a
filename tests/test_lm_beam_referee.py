"""The referees of tests/lm_beam_referee.py, proved on the CPU:

* chained and run with one utterance they ARE the host BeamSearchLM on the toy LM of
  tests/golden/beam_lm.npz (letters, mappings, finished list and bags exactly, scores to 1e-5);
* the case matrix (single launches, tie cases, the 12-step trajectory) tells each single-term
  mutant from the real thing, and every case has its margins above decode_referee.MARGIN_FLOOR;
* the identity the kernels rely on: the cost of an extension from arc_w_closed = weight - log Z(dst)
  equals the host's expand + closure + reduce, and the survivors' bags equal BeamSearchLM._Bags.get,
  on the toy LM and both shipped character LMs."""
import numpy as np
import pytest
import torch

import decode_referee as dr
import lm_beam_referee as lr
from conftest import golden


def _host(g, lm, cfg, beam, C, keep):
    from att_speech.modules.beam_search import BeamSearchLM
    return BeamSearchLM(lm, cfg['lm_weight'], g['mapping'].tolist(), cfg['min_attention_pos'],
                        cfg['coverage_tau'], cfg['coverage_weight'], 1, beam, torch.device('cpu'), C,
                        cfg['ln'], keep_eos_score=keep)


@pytest.mark.parametrize('cfg', [dict(lm_weight=0.5, min_attention_pos=0.3, coverage_tau=0.1, coverage_weight=0.2, ln=0.6, keep=False),
                                 dict(lm_weight=0.8, min_attention_pos=0.2, coverage_tau=0.1, coverage_weight=0.0, ln=0.0, keep=True)],
                         ids=['lm', 'lm_keep_eos'])
def test_referee_step_by_step_is_the_host_class(cfg):
    g = golden('beam_lm.npz')
    lm, C, beam = lr.toy_lm(), 7, 4
    steps, T = g['logits'].shape[0], g['att'].shape[1]
    host = _host(g, lm, cfg, beam, C, cfg['keep'])
    params = {k: cfg[k] for k in ('lm_weight', 'min_attention_pos', 'coverage_tau', 'coverage_weight')}
    rs = lr.RefSearch(lm, g['mapping'].tolist(), 1, beam, C, T, [T], steps + 1, keep_eos=cfg['keep'], **params)
    lr_ln, lr.LN = lr.LN, cfg['ln']
    try:
        for s in range(steps):
            letters, mapping = host.step(torch.from_numpy(g['logits'][s][:, :beam]).clone(),
                                         att_weights=torch.from_numpy(g['att'][s][:, :beam]).clone())
            out, _ = rs.step(g['logits'][s][0, :beam] if g['logits'][s].ndim == 3 else g['logits'][s][:beam],
                             np.ascontiguousarray(g['att'][s][:, :beam].T))
            np.testing.assert_array_equal(out['new_input'], letters.numpy())
            np.testing.assert_array_equal(out['parent'], mapping.numpy())
            hs = host.scores.numpy()
            assert np.array_equal(np.isfinite(out['scores_out']), np.isfinite(hs))
            np.testing.assert_allclose(out['scores_out'][np.isfinite(hs)], hs[np.isfinite(hs)], rtol=1e-5, atol=1e-5)
            np.testing.assert_array_equal(rs.est[:, :s + 1], host.estimations.numpy())
            # bags exactly (same states; costs to the last bits of two summation orders)
            assert [sorted(d) for d in rs.bags] == [sorted(d) for d in host.fst_states]
            for a, b in zip(rs.bags, host.fst_states):
                np.testing.assert_allclose([a[k] for k in sorted(a)], [b[k] for k in sorted(b)], rtol=1e-12)
            # the finished list
            st = rs.state
            p, n = st['fin_parity'][0], st['fin_count'][0]
            assert n == len(host.finished)
            np.testing.assert_allclose(st['fin_score'][p, 0, :n], [float(f[0]) for f in host.finished], rtol=1e-5)
            assert st['fin_beam'][p, 0, :n].tolist() == [int(f[2]) for f in host.finished]
            for r, f in enumerate(host.finished):
                assert st['fin_tokens'][p, 0, r, :st['fin_len'][p, 0, r]].tolist() == f[1].tolist()
            if host.coverage is not None:
                np.testing.assert_allclose(rs.cov.T, host.coverage.numpy(), rtol=1e-6)
            if host.has_finished():
                assert st['frozen'][0] == 1
                break
            assert st['frozen'][0] == 0
    finally:
        lr.LN = lr_ln
    st = rs.state
    if st['best_len'][0]:
        assert st['best_tokens'][0, :st['best_len'][0]].tolist() == host.best_finished[0].tolist()
        np.testing.assert_allclose(st['best_score'][0], float(host.best_finished_scores[0]), rtol=1e-5)
        for i, k in enumerate(('acoustic', 'lm', 'coverage')):
            if k in host.best_finished_scores_elements:
                np.testing.assert_allclose(st['best_elems'][0, i], host.best_finished_scores_elements[k][0],
                                           rtol=1e-5, atol=1e-6)


def _trajectory(mut=None, dtype=np.float64):
    t = lr.TRAJ
    logits, att = lr.traj_inputs(**t)
    rs = lr.RefSearch(lr.toy_lm(), lr.TOY_MAPPING, t['B'], t['beam'], t['C'], lr.T_FRAMES, t['lens'],
                      t['steps'] + 1, keep_eos=True, dtype=dtype, mut=mut)
    outs = [rs.step(logits[s], att[s]) for s in range(t['steps'])]
    return rs, outs


def test_every_case_has_clear_margins():
    for case in lr.SINGLE_CASES:
        c = lr.single_case(*case)
        want, m = lr.lm_beam_step_ref(c)
        tol, _ = lr.tolerance(c, want)
        assert lr.min_margin(m) > dr.MARGIN_FLOOR, (case, m)
        assert 10 * tol <= dr.MARGIN_FLOOR, (case, tol)
        # the fp32 run of the referee decides as the fp64 one and passes its own judge
        f32, _ = lr.lm_beam_step_ref(c, dtype=np.float32)
        assert lr.judge(c, lr.kernel_view(c, f32), want, tol) == [], case
    rs, outs = _trajectory()
    assert min(lr.min_margin(m) for m in rs.margins) > dr.MARGIN_FLOOR
    frozen = [o['frozen'].tolist() for o, _ in outs]
    assert frozen[1] == [0, 0, 0] and frozen[2] == [0, 1, 1] and frozen[-1] == [1, 1, 1]   # one runs on alone


def test_tie_cases_decide_by_the_stated_rules():
    t = lr.tie_cases()
    o, _ = lr.lm_beam_step_ref(t['lowest_flat_index_wins'])
    assert o['parent'].tolist() == [0, 1, 2] and o['new_input'].tolist() == [0, 0, 0]
    o, _ = lr.lm_beam_step_ref(t['first_step_equal'])
    assert o['parent'].tolist() == [0, 0] and o['new_input'].tolist() == [0, 1]
    for mut, order in ((None, [0, 1]), ('newest_first_on_ties', [1, 0])):
        c1 = t['finish_beam_0']
        o1, _ = lr.lm_beam_step_ref(c1, dtype=np.float32, mut=mut)
        assert o1['fin_count'].tolist() == [1] and o1['improved'].tolist() == [True]
        c2 = lr.tie_second_launch(c1, {k: o1[k] for k in lr.STATE_KEYS})
        o2, _ = lr.lm_beam_step_ref(c2, dtype=np.float32, mut=mut)
        p = o2['fin_parity'][0]
        assert o2['fin_count'].tolist() == [2] and o2['fin_beam'][p, 0, :2].tolist() == order
        assert o2['fin_score'][p, 0, 0] == o2['fin_score'][p, 0, 1]                  # an exact tie
        assert o2['added'].tolist() == [True] and o2['improved'].tolist() == [False]   # equal does not replace
        assert o2['best_tokens'][0, 0] == c1['est_in'][0, 0] != c1['est_in'][1, 0]


@pytest.mark.parametrize('mut', lr.MUTANTS)
def test_case_matrix_tells_the_mutant_apart(mut):
    caught = []
    if mut in ('z_omitted', 'closure_before_label'):
        for case in lr.SINGLE_CASES:
            c = lr.single_case(*case)
            bad = lr.label_costs_ref(c['lm'], c['bags'], c['mapping'], c['C'], mut)
            fin = np.isfinite(c['lm_cost'])
            if not np.array_equal(fin, np.isfinite(bad)) or \
                    (np.abs(bad[fin] - c['lm_cost'][fin]) > 1e-9 * np.abs(c['lm_cost'][fin])).any():
                caught.append(case)
    else:
        cases = [(k, lr.single_case(*k)) for k in lr.SINGLE_CASES] + sorted(lr.tie_cases().items())
        for key, c in cases:
            want, _ = lr.lm_beam_step_ref(c)
            got, _ = lr.lm_beam_step_ref(c, mut=mut)
            if lr.judge(c, lr.kernel_view(c, got), want, lr.tolerance(c, want)[0]):
                caught.append(key)
        # the exact two-launch tie (fp32 throughout, so that the second score repeats the first bit for bit)
        c1 = lr.tie_cases()['finish_beam_0']
        o1, _ = lr.lm_beam_step_ref(c1, dtype=np.float32)
        c2 = lr.tie_second_launch(c1, {k: o1[k] for k in lr.STATE_KEYS})
        want, _ = lr.lm_beam_step_ref(c2, dtype=np.float32)
        got, _ = lr.lm_beam_step_ref(c2, dtype=np.float32, mut=mut)
        if lr.judge(c2, lr.kernel_view(c2, got), want, lr.tolerance(c2, want)[0]):
            caught.append('tie_second_launch')
        rs, outs = _trajectory()
        ms, mouts = _trajectory(mut)
        for s, ((want, c), (got, _)) in enumerate(zip(outs, mouts)):
            if lr.judge(c, lr.kernel_view(c, got), want, lr.tolerance(c, want)[0]):
                caught.append(('trajectory', s))
                break
    assert caught, mut


# ------------------------------------------------------------------ the Z(n) identity

def _random_bags(lm, mapping, C, gen, n):
    bags = []
    for _ in range(n):
        k = int(torch.randint(0, 5, (1,), generator=gen))
        labs = [mapping[int(v)] for v in torch.randint(0, C - 1, (k,), generator=gen)]
        bag = lr.walk_bag(lm, labs)
        shift = float(torch.rand(1, generator=gen)) * 30
        bags.append({s: w + shift for s, w in sorted(bag.items())})
    return bags


@pytest.mark.parametrize('name', ['toy', 'bg', 'tg'])
def test_closed_arc_weights_give_the_cost_of_the_closed_bag(name):
    from att_speech import fst_utils as P
    from att_speech.modules.beam_search import BeamSearchLM
    C = 7 if name == 'toy' else 52
    lm, mapping = lr.case_lm(name, C)
    gen = torch.Generator().manual_seed(3)
    bags = _random_bags(lm, mapping, C, gen, 12)
    assert max(len(b) for b in bags) >= 2
    want = lr.label_costs_ref(lm, bags, mapping, C)
    wc = lm.arc_w_closed()
    got = np.full((len(bags), C), np.inf)
    for h, bag in enumerate(bags):
        for c in range(C):
            terms = []
            for s, w in bag.items():
                lo, hi = int(lm.ptr[s]), int(lm.ptr[s + 1])
                a = lo + np.searchsorted(lm.ilabel[lo:hi], [mapping[c], mapping[c] + 1])
                terms += (w + wc[a[0]:a[1]]).tolist()
            got[h, c] = P.reduce_weights(terms, True)
    fin = np.isfinite(want)
    assert fin.any() and np.array_equal(fin, np.isfinite(got))
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12)
    # survivors' bags: the referee's expand is what BeamSearchLM._Bags.get hands out
    search = BeamSearchLM.__new__(BeamSearchLM)
    search.lm, search.fst_states, search.beam_size = lm, bags, len(bags)
    search.num_classes, search.alphabet_mapping, search.lm_weight = C, mapping, 1.0
    _, all_states = search._step_lm()
    letters = torch.randint(0, C - 1, (len(bags),), generator=gen).tolist()
    mine = lr.bag_advance_ref(lm, bags, range(len(bags)), letters, mapping)
    for h, l in enumerate(letters):
        host = all_states.get(h, l)
        assert sorted(host) == sorted(mine[h])
        np.testing.assert_allclose([mine[h][k] for k in sorted(host)], [host[k] for k in sorted(host)], rtol=1e-12)


def test_lm_with_an_epsilon_cycle_has_no_closed_weights():
    from att_speech.lm_fst import LmFst
    lm = LmFst(4, 0, [0, 1, 2, 3], [1, 2, 1, 3], [1, 0, 0, 1], [1, 0, 0, 1], [0.5, 0.1, 0.2, 0.3], np.zeros(4))
    assert lm.arc_w_closed() is None and lm.device_arrays('cpu') is None
