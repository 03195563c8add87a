"""The three kernels of a beam-search label step, one launch at a time against the fp64 referees
of tests/decode_referee.py (proved on the CPU by tests/test_decode_referee.py, which also shows
that this matrix catches each of ten one-term mutants): asr_beam_step_f32,
asr_tcn_attention_step_f32 and asr_att_gru_scan_fwd_f32 with L = 1, beam > 1, save = False.

Beam step.  Integer outputs are bit-equal to the referee at every case; every case is seeded so
that each live decision has a margin above 1e-3 (asserted), or is an exact tie case.  Scores are
held to 4x the distance of an fp32 CPU evaluation of the same step (torch.log_softmax + add)
from fp64 plus 4 fp32 ulps of the largest operand.  Measured, MI355X, maxima over the steps
{0, 1, 7, 11} of each shape (B, beam, C): fp32 CPU distance / kernel error / tolerance, and the
smallest margin

    (1,1,2)    3.1e-06 / 3.1e-06 / 5.2e-05   13        (3,3,5)    4.7e-06 / 4.7e-06 / 6.7e-05   0.53
    (2,10,50)  5.8e-06 / 5.8e-06 / 8.2e-05   0.0023    (1,32,65)  6.2e-06 / 6.2e-06 / 8.3e-05   0.0052
    (4,8,4)    5.9e-06 / 5.9e-06 / 8.4e-05   0.039     (5,32,3)   6.0e-06 / 6.0e-06 / 8.5e-05   0.0066
    (7,10,50)  3.5e-06 / 3.8e-06 / 7.3e-05   0.0033    (2,16,129) 3.3e-06 / 3.8e-06 / 7.2e-05   0.0065
    (3,32,65)  6.3e-06 / 6.3e-06 / 8.4e-05   0.0027    (40,4,7)   6.2e-06 / 6.2e-06 / 8.5e-05   0.011
    (2,32,9)   4.9e-06 / 4.9e-06 / 7.8e-05   0.0029

(both errors are a few ulps of scores near -100 .. -250).  The margin floor of 1e-3 is more than
10x above every error and every tolerance (asserted per case).  The 12-step sequences have
margins from 0.0016 ((3,32,65)) to 19.5.

Attention steps.  4x the fp32 evaluation's distance from fp64 plus the term of the kernels'
exp form of tanh (decode_referee.TANH_ABS = 2^-21; measured through the kernel: 4.3e-07 for the
difference of two values, softmax included).  Measured maxima over the cases, fp32 distance /
kernel error / tolerance range: local attention alignment 2.0e-07 / 1.3e-07 / 4.9e-07 .. 1.8e-05,
context 1.0e-06 / 5.2e-07 / 4.8e-06 .. 8.3e-05; attention-GRU alignment 1.2e-07 / 8.0e-08 /
1.0e-06 .. 7.0e-06, states 3.5e-07 / 2.5e-07 / 9.3e-07 .. 2.1e-06.

What this file found: the kernel before it counted a dead hypothesis (running score -inf) whose
flat row the EOS quirk reads as "EOS is best" from its logits, where the host class sees a row of
-inf and class 0 (finished_count wrong at (3,3,5) step 1, (5,32,3) step 11, (40,4,7) steps 1, 7,
11 and in the (4,8,4) sequence), and filled the slots that finite candidates leave with copies of
the last finite index instead of the -inf candidates in index order (the (5,32,3) sequence)."""
import numpy as np
import pytest
import torch

import decode_referee as dr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def native():
    from att_speech import _native
    return _native


# ---------------------------------------------------------------- beam step: one launch

def device_buffers(c, est_prefill=dr.POISON):
    hyps = c['B'] * c['beam']
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    state = {k: t(v) for k, v in c['state'].items()}
    state['best_score'] = state['best_score'].float()
    state['new_input'] = torch.full((hyps,), dr.POISON, dtype=torch.int32, device=DEV)
    state['parent'] = torch.full((hyps,), dr.POISON, dtype=torch.int32, device=DEV)
    return dict(logits=t(c['logits']), scores_in=t(c['scores_in']),
                scores_out=torch.full((hyps,), float('nan'), device=DEV), est_in=t(c['est_in']),
                est_out=torch.full((hyps, c['Lcap']), est_prefill, dtype=torch.int32, device=DEV),
                state=state)


def launch(c, d):
    native().beam_step(d['logits'], d['scores_in'], d['scores_out'], d['est_in'], d['est_out'],
                       c['step'], c['B'], c['beam'], c['len_div'], d['state'])
    torch.cuda.synchronize()
    got = {k: d['state'][k].cpu().numpy() for k in ('finished_count', 'best_score', 'best_len',
                                                    'best_tokens', 'done', 'new_input', 'parent')}
    got.update(est_out=d['est_out'].cpu().numpy(), scores_out=d['scores_out'].cpu().numpy())
    return got


def ref(c, **kw):
    return dr.beam_step_ref(c['logits'], c['scores_in'], c['est_in'], c['step'], c['B'], c['beam'],
                            c['len_div'], c['state'], **kw)


def score_error(got, want):
    fin = np.isfinite(want['scores_out'])
    err = np.abs(got['scores_out'][fin] - want['scores_out'][fin]).max(initial=0.0)
    imp = want['improved']
    return max(float(err), float(np.abs(got['best_score'][imp] - want['best_score'][imp]).max(initial=0.0)))


@pytest.mark.parametrize('case', dr.SINGLE_CASES, ids=str)
def test_beam_step_from_arbitrary_state(case):
    c = dr.single_case(*case)
    want, margins = ref(c)
    tol, d32 = dr.beam_tolerance(c, want)
    got = launch(c, device_buffers(c))
    err = score_error(got, want)
    print('%s smallest margin %.3g  fp32 distance %.3g  kernel error %.3g  tolerance %.3g' % (
        case, dr.min_margin(margins), d32, err, tol))
    assert dr.min_margin(margins) > dr.MARGIN_FLOOR             # every decision of the case is clear
    assert 10 * max(err, tol) <= dr.MARGIN_FLOOR
    assert dr.judge_beam_step(c, got, want, tol) == []


@pytest.mark.parametrize('name', sorted(dr.tie_cases()))
def test_beam_step_ties(name):
    c = dr.tie_cases()[name]
    want, _ = ref(c)
    got = launch(c, device_buffers(c))
    assert dr.judge_beam_step(c, got, want, dr.beam_tolerance(c, want)[0]) == []


def test_best_score_equal_to_the_candidate_stays():
    c = dr.tie_cases()['equal_eos_scores']                      # step 1: normalised = raw
    first = launch(c, device_buffers(c))
    assert first['best_len'].tolist() == [1] and np.isfinite(first['best_score']).all()
    again = dict(c, state=dict(c['state'], best_score=first['best_score']))
    got = launch(again, device_buffers(again))
    assert got['finished_count'].tolist() == [1] and got['best_len'].tolist() == [0]
    assert (got['best_tokens'] == dr.POISON).all()
    assert got['best_score'].tobytes() == first['best_score'].tobytes()


def test_beam_step_argument_checks_launch_nothing():
    c = dr.single_case(3, 3, 5, 1)

    def refused(exc, **kw):
        cc = dict(c, **kw)
        d = device_buffers(cc)
        with pytest.raises(exc):
            launch(cc, d)
        torch.cuda.synchronize()
        assert bool((d['est_out'] == dr.POISON).all()) and bool(torch.isnan(d['scores_out']).all())
        assert d['state']['done'].cpu().tolist() == [0, 0, 1]

    big = dr.beam_case(1, 33, 5, 1, 0)
    refused(NotImplementedError, **{k: big[k] for k in ('logits', 'scores_in', 'est_in', 'beam', 'state')})
    wide = dr.beam_case(1, 1, 2050, 1, 0)                        # beam * (C - 1) = 2049
    refused(NotImplementedError, **{k: wide[k] for k in ('logits', 'scores_in', 'est_in', 'beam', 'B', 'state')})
    refused(AssertionError, step=dr.SINGLE_LCAP)                 # Lcap == step


# ---------------------------------------------------------------- beam step: sequences

def _snapshot(search):
    return [t.clone() for t in search._scores + search._est] + [v.clone() for v in search._state.values()]


@pytest.mark.parametrize('shape', sorted(dr.TRAJECTORIES), ids=str)
def test_device_beam_search_step_by_step(shape):
    """12 launches through DeviceBeamSearch; the referee restarts from the device's own state at
    every step, so that rounding does not accumulate."""
    from att_speech.modules.beam_search import DeviceBeamSearch
    B, beam, C = shape
    steps = dr.TRAJECTORY_STEPS
    logits = dr.beam_logits(B, beam, C, dr.TRAJECTORIES[shape], steps)
    search = DeviceBeamSearch(B, beam, torch.device(DEV), C, dr.LENGTH_NORMALIZATION, steps)
    worst = float('inf')
    for s in range(steps):
        keys = ('finished_count', 'best_score', 'best_len', 'best_tokens', 'done')
        c = dict(logits=logits[s], scores_in=search._scores[s & 1].cpu().numpy(),
                 est_in=search._est[s & 1].cpu().numpy(), step=s, B=B, beam=beam, C=C, Lcap=steps + 1,
                 len_div=dr.len_div(s), state={k: search._state[k].cpu().numpy() for k in keys})
        before = search._est[(s + 1) & 1].cpu().numpy()
        want, margins = ref(c)
        search.step(torch.from_numpy(logits[s]).to(DEV))
        torch.cuda.synchronize()
        got = {k: search._state[k].cpu().numpy() for k in keys + ('new_input', 'parent')}
        got.update(est_out=search._est[(s + 1) & 1].cpu().numpy(), scores_out=search._scores[(s + 1) & 1].cpu().numpy())
        if want['noop']:
            got.update(scores_out=None)
        worst = min(worst, dr.min_margin(margins))
        assert dr.min_margin(margins) > dr.MARGIN_FLOOR, (s, margins)
        assert dr.judge_beam_step(c, got, want, dr.beam_tolerance(c, want)[0], est_before=before) == [], s
    print('%s smallest margin over %d steps %.3g' % (shape, steps, worst))


def test_launches_after_the_flag_change_nothing_and_finalize_is_the_host_class():
    from att_speech.modules.beam_search import BeamSearch, DeviceBeamSearch
    (B, beam, C), seed, bias = dr.FINISHING
    steps = dr.TRAJECTORY_STEPS
    logits = dr.beam_logits(B, beam, C, seed, steps, bias)
    res = dr.run_trajectory(B, beam, C, logits)
    assert min(dr.min_margin(m) for _, m in res) > dr.MARGIN_FLOOR
    host = BeamSearch(B, beam, torch.device('cpu'), C, dr.LENGTH_NORMALIZATION)
    stop = None
    for s in range(steps):
        host.step(torch.from_numpy(logits[s])[None])
        if host.has_finished():
            stop = s + 1
            break
    assert stop is not None and stop <= 7
    search = DeviceBeamSearch(B, beam, torch.device(DEV), C, dr.LENGTH_NORMALIZATION, steps)
    for s in range(steps):
        frozen = _snapshot(search) if s >= stop else None
        search.step(torch.from_numpy(logits[s]).to(DEV))
        torch.cuda.synchronize()
        assert search.poll_finished() == (s + 1 >= stop)
        if frozen is not None:                                   # no byte of any buffer changes
            for a, b in zip(frozen, _snapshot(search)):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert int(search._state['done'][2]) == min(s + 1, stop)
    search.finalize()
    assert search.finished_count == host.finished_count
    assert [[int(v) for v in t] for t in search.best_finished] == [[int(v) for v in t] for t in host.best_finished]
    np.testing.assert_allclose(search.best_finished_scores, host.best_finished_scores, rtol=1e-5)
    live = np.isfinite(host.scores.numpy())
    assert np.array_equal(np.isfinite(search.scores.cpu().numpy()), live)
    np.testing.assert_array_equal(search.estimations.cpu().numpy()[live], host.estimations.numpy()[live])
    np.testing.assert_allclose(search.scores.cpu().numpy()[live], host.scores.numpy()[live], rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- local-attention step

@pytest.mark.parametrize('key', dr.ATT_CASES, ids=str)
def test_local_attention_step(key):
    c = dr.att_case(*key)
    want = dr.tcn_attention_step_ref(*dr.att_args(c))
    tols = dr.att_tolerance(c, want)
    att, ctx = native().tcn_attention_step(*dr.att_args(c, DEV))
    att, ctx = att.cpu(), ctx.cpu()
    print('%s fp32 distance att %.3g ctx %.3g  kernel error att %.3g ctx %.3g  tolerance %.3g %.3g' % (
        key, tols[2], tols[3], float((att.double() - want[0]).abs().max()),
        float((ctx.double() - want[1]).abs().max()), tols[0], tols[1]))
    assert not torch.isnan(att).any() and not torch.isnan(ctx).any()
    assert dr.judge_att_step(c, att, ctx, want, tols) == []


def test_exp_form_of_tanh_is_within_its_term():
    """A = 1, w = 1, no filter: the alignment is softmax_t(tanh(x_t)), so log a_t - log a_0 is
    tanh(x_t) - tanh(x_0) up to two relative errors of the softmax (2^-22 each)."""
    T = 256
    x = torch.linspace(-9, 9, T)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    att, _ = native().tcn_attention_step(
        x.view(T, 1, 1).to(DEV), z(T, 1, 4), torch.tensor([T], dtype=torch.int32, device=DEV),
        z(1, 1, 32), z(1, 1), torch.ones(1, device=DEV), 0.0, 1.0, torch.full((1, T), 1.0 / T, device=DEV), None, 1)
    la = att[0].cpu().double().log()
    th = torch.tanh(x.double())
    err = float(((la - la[0]) - (th - th[0])).abs().max())
    print('exp form of tanh through the kernel: %.3g (TANH_ABS %.3g)' % (err, dr.TANH_ABS))
    assert err <= 2 * dr.TANH_ABS + 2.0 ** -21


def test_local_attention_step_refuses_what_does_not_fit_lds():
    T = dr.ATT_STEP_MAX_FRAMES + 1
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(NotImplementedError):
        native().tcn_attention_step(z(T, 1, 4), z(T, 1, 4), torch.tensor([T], dtype=torch.int32, device=DEV),
                                    z(1, 4, 32), z(1, 4), z(4), 0.0, 1.0, z(1, T), None, 1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- attention-GRU step as decode uses it

@pytest.mark.parametrize('shape', dr.GRU_SHAPES, ids=str)
def test_attention_gru_step_with_beam(shape):
    c = dr.gru_case(shape)
    beam = c['beam']
    assert native().att_gru_supported(shape[0], shape[3], shape[4], shape[5])
    want = dr.att_gru_step_ref(*dr.gru_args(c), beam)
    tols = dr.gru_tolerance(c, want)
    a = dict(zip(dr.GRU_KEYS, dr.gru_args(c, DEV)))

    def run(eproj, encoded, lens, beam):
        return native().att_gru_scan_fwd(eproj, encoded, lens, a['gx_emb'][None], a['w_ic'], a['w_hh'],
                                         a['b_hh'], a['w_rec'], a['w_score'], a['b_score'], a['h0'],
                                         beam=beam, save=False)
    att, states, ctxs, gates, rec = run(a['eproj'], a['encoded'], a['lens'], beam)
    assert ctxs is None and gates is None and rec is None
    got_att, got_states = att[0].cpu(), states[0].cpu()
    print('%s fp32 distance att %.3g states %.3g  kernel error att %.3g states %.3g  tolerance %.3g %.3g' % (
        shape, tols[2], tols[3], float((got_att.double() - want[0]).abs().max()),
        float((got_states.double() - want[1]).abs().max()), tols[0], tols[1]))
    assert dr.judge_gru_step(c, got_att, got_states, want, tols) == []
    # the same hypotheses with every operand repeated per hypothesis: bitwise (fixed reduction order)
    att1, states1, _, _, _ = run(a['eproj'].repeat_interleave(beam, 1).contiguous(),
                                 a['encoded'].repeat_interleave(beam, 1).contiguous(),
                                 a['lens'].repeat_interleave(beam).contiguous(), 1)
    assert torch.equal(att1, att) and torch.equal(states1, states)
