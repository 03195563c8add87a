"""The fp64 referees of tests/decode_referee.py, proved on the CPU before they judge a kernel
(tests/test_decode_step_gpu.py):

* `beam_step_ref`, free-running over 12 steps from fresh state, is the host BeamSearch class
  (pinned to the upstream golden by test_tcn_beam.py) at every step: labels, mapping,
  estimations, finished_count, best_finished, best_finished_scores (scores to rtol 1e-5), with
  every decision margin above 1e-3 at the committed seeds;
* every single-launch case of the GPU matrix has all its margins above 1e-3, and the distance of
  the fp32 evaluation from fp64, the measure of the kernel's tolerance, stays 10x below that;
* `tcn_attention_step_ref` is LocalAttention.forward + enc_step's context in double, and
  `att_gru_step_ref` is AttentionDecoderRNN._step in double, to 1e-10;
* the same arithmetic in fp32 passes the judges at every case: the tolerance is not too tight;
* each mutant, one wrong term of the reference standing in for the kernel, is caught by the
  judges at one case of the GPU matrix at least.

Measured on the CPU, cases of the GPU matrix that catch each mutant (beam step: 44 single
launches + 6 tie cases; attention step: 16; attention-GRU step: 5):

    mutant                     kernel      caught at
    eos_row_b_times_beam       beam step   13 cases
    count_below_beam           beam step    8
    normalised_score_stored    beam step    7
    highest_index_on_ties      beam step    6   (the tie cases and no other, as it must be)
    first_step_all_beams       beam step   10
    padding_repeats_index_0    beam step    3   ((4,8,4), (5,32,3) and (2,32,9) at step 0)
    parent_ignored             attention    4
    mask_after_len             attention   11
    u_is_b_mod_nu              att-GRU      4
    len_0_is_empty             att-GRU      5
"""
import types

import numpy as np
import pytest
import torch

import decode_referee as dr
from decode_referee import F64


# ---------------------------------------------------------------- the referee is the host class

@pytest.mark.parametrize('shape', sorted(dr.TRAJECTORIES), ids=str)
def test_beam_referee_is_the_host_class(shape):
    from att_speech.modules.beam_search import BeamSearch
    B, beam, C = shape
    logits = dr.beam_logits(B, beam, C, dr.TRAJECTORIES[shape], dr.TRAJECTORY_STEPS)
    res = dr.run_trajectory(B, beam, C, logits)
    worst = min(dr.min_margin(m) for _, m in res)
    print('%s seed %d: smallest margin %.3g' % (shape, dr.TRAJECTORIES[shape], worst))
    assert worst > dr.MARGIN_FLOOR
    host = BeamSearch(B, beam, torch.device('cpu'), C, dr.LENGTH_NORMALIZATION)
    compared = 0
    for s, (out, _) in enumerate(res):
        assert not out['noop']
        labels, mapping = host.step(torch.from_numpy(logits[s])[None])
        live = np.isfinite(out['scores_out'])
        hs = host.scores.numpy()
        assert np.array_equal(np.isfinite(hs), live)                # dead slots are dead on both sides
        # (atol: one fp32 ulp of the largest logit, for a score that is 0 in fp32 and -4e-15 in fp64)
        atol = dr.EPS32 * float(np.abs(logits[s]).max())
        np.testing.assert_allclose(hs[live], out['scores_out'][live], rtol=1e-5, atol=atol)
        np.testing.assert_array_equal(labels.numpy()[live], out['new_input'][live])
        np.testing.assert_array_equal(mapping.numpy()[live], out['parent'][live])
        np.testing.assert_array_equal(host.estimations.numpy()[live], out['est'][live])
        assert host.finished_count == out['finished_count'].tolist()
        for b in range(B):
            got = [int(v) for v in host.best_finished[b]]
            assert got == out['best_tokens'][b, :out['best_len'][b]].tolist()
        np.testing.assert_allclose(np.array(host.best_finished_scores), out['best_score'], rtol=1e-5, atol=atol)
        assert host.has_finished() == bool(out['done'][0])
        assert out['done'][2] == s + 1
        compared += 1
        if host.has_finished():
            break
    assert compared >= 2
    if compared < len(res):                                          # after the flag: no-ops
        assert res[compared][0]['noop']


def test_padding_shapes_take_the_padding_path():
    for shape in ((4, 8, 4), (5, 32, 3)):
        B, beam, C = shape
        res = dr.run_trajectory(B, beam, C, dr.beam_logits(B, beam, C, dr.TRAJECTORIES[shape], 3))
        assert np.isinf(res[0][0]['scores_out']).sum() == B * (beam - (C - 1))
        assert np.isinf(res[1][0]['scores_out']).any() == ((C - 1) ** 2 < beam)
    assert 32 * 64 == 2048                                           # (3, 32, 65): the capacity


# ---------------------------------------------------------------- the single-launch matrix

def _ref(c, **kw):
    return dr.beam_step_ref(c['logits'], c['scores_in'], c['est_in'], c['step'], c['B'], c['beam'],
                            c['len_div'], c['state'], **kw)


@pytest.mark.parametrize('case', dr.SINGLE_CASES, ids=str)
def test_single_launch_cases_have_clear_margins(case):
    c = dr.single_case(*case)
    want, m = _ref(c)
    tol, d32 = dr.beam_tolerance(c, want)
    print('%s margins %s  fp32 distance %.3g  tolerance %.3g' % (
        case, {k: float('%.3g' % v) for k, v in m.items()}, d32, tol))
    assert dr.min_margin(m) > dr.MARGIN_FLOOR
    assert 10 * tol <= dr.MARGIN_FLOOR
    f32, _ = _ref(c, dtype=np.float32)
    assert dr.judge_beam_step(c, dr.kernel_view(c, f32), want, tol) == []


def test_the_single_launch_matrix_reaches_every_branch():
    seen = dict(inf_in=0, pad=0, improved=0, kept_above=0, capped=0, at_beam=0, dead_quirk_row=0)
    for case in dr.SINGLE_CASES:
        c = dr.single_case(*case)
        want, _ = _ref(c)
        B, beam, step = c['B'], c['beam'], c['step']
        fc0 = c['state']['finished_count']
        seen['inf_in'] += bool(np.isinf(c['scores_in']).any())
        seen['pad'] += bool(np.isinf(want['scores_out']).any())
        seen['improved'] += bool(want['improved'].any())
        seen['kept_above'] += bool(step and ((want['finished_count'] > fc0) & ~want['improved']).any())
        seen['capped'] += bool(step and (fc0 == beam + 1).any())
        seen['at_beam'] += bool(step and ((fc0 == beam) & (want['finished_count'] == beam + 1)).any())
        seen['dead_quirk_row'] += bool(step and np.isinf(c['scores_in'][:B]).any())
    print(seen)
    assert all(v >= 3 for v in seen.values()), seen


def test_tie_cases_follow_the_stable_sort_and_first_maximum_rules():
    t = dr.tie_cases()
    w = {k: _ref(c)[0] for k, c in t.items()}
    # a row of equal logits: candidates 0..3 of beam 0 tie, the best of beam 1 (class 3) is first
    assert w['all_equal_row']['parent'].tolist() == [1, 0] and w['all_equal_row']['new_input'].tolist() == [3, 0]
    assert w['all_equal_everywhere']['parent'].tolist() == [0, 0, 0, 3, 3, 3]
    assert w['all_equal_everywhere']['new_input'].tolist() == [0, 1, 2, 0, 1, 2]
    assert w['all_equal_everywhere']['finished_count'].tolist() == [0, 0]      # EOS ties: class 0 is the argmax
    # identical rows: beam 0 before beam 1 before beam 2 at the best class
    assert w['identical_rows']['parent'].tolist() == [0, 1, 2] and w['identical_rows']['new_input'].tolist() == [0, 0, 0]
    # EOS equal to the best other class of flat row b (rows 0 and 1): utterance 0 does not finish,
    # utterance 1 (row 1: EOS alone on top) does
    c = t['eos_equals_best_class']
    assert int(torch.argmax(torch.from_numpy(c['logits'][0]))) == 0
    assert w['eos_equals_best_class']['finished_count'].tolist() == [0, 1]
    # equal normalised EOS scores: the first beam's history is kept
    c = t['equal_eos_scores']
    assert w['equal_eos_scores']['improved'].tolist() == [True]
    assert w['equal_eos_scores']['best_tokens'][0, :1].tolist() == c['est_in'][0, :1].tolist()
    assert c['est_in'][0, 0] != c['est_in'][1, 0]
    assert w['first_step_equal']['parent'].tolist() == [0, 0] and w['first_step_equal']['new_input'].tolist() == [0, 1]
    # best_score equal to the candidate: no update
    c = dict(t['equal_eos_scores'])
    c['state'] = dict(c['state'], best_score=w['equal_eos_scores']['best_score'].astype(np.float64))
    again, m = _ref(c)
    assert m['best_vs_eos'] == 0 and not again['improved'].any() and (again['best_tokens'] == dr.POISON).all()
    for k, c in t.items():
        f32, _ = _ref(c, dtype=np.float32)
        assert dr.judge_beam_step(c, dr.kernel_view(c, f32), w[k], dr.beam_tolerance(c, w[k])[0]) == [], k


# ---------------------------------------------------------------- mutants

def _beam_matrix():
    return [(str(k), dr.single_case(*k)) for k in dr.SINGLE_CASES] + sorted(dr.tie_cases().items())


def caught_by(mut):
    """names of the cases of the GPU matrix at which the mutant, standing in for the kernel, fails"""
    hit = []
    if mut in dr.BEAM_MUTANTS:
        for name, c in _beam_matrix():
            want, _ = _ref(c)
            got, _ = _ref(c, mut=mut)
            if dr.judge_beam_step(c, dr.kernel_view(c, got), want, dr.beam_tolerance(c, want)[0]):
                hit.append(name)
    elif mut in dr.ATT_MUTANTS:
        for key in dr.ATT_CASES:
            c = dr.att_case(*key)
            want = dr.tcn_attention_step_ref(*dr.att_args(c))
            got = dr.tcn_attention_step_ref(*dr.att_args(c), mut=mut)
            if dr.judge_att_step(c, got[0], got[1], want, dr.att_tolerance(c, want)):
                hit.append(str(key))
    else:
        for shape in dr.GRU_SHAPES:
            c = dr.gru_case(shape)
            want = dr.att_gru_step_ref(*dr.gru_args(c), c['beam'])
            got = dr.att_gru_step_ref(*dr.gru_args(c), c['beam'], mut=mut)
            if dr.judge_gru_step(c, got[0], got[1], want, dr.gru_tolerance(c, want)):
                hit.append(str(shape))
    return hit


@pytest.mark.parametrize('mut', dr.BEAM_MUTANTS + dr.ATT_MUTANTS + dr.GRU_MUTANTS)
def test_mutant_is_caught_by_the_gpu_matrix(mut):
    hit = caught_by(mut)
    print('%-26s caught at %2d cases: %s' % (mut, len(hit), ', '.join(hit[:6])))
    assert hit
    if mut == 'highest_index_on_ties':          # no other case may depend on the tie rule
        assert set(hit) <= set(dr.tie_cases())


# ---------------------------------------------------------------- the other two referees

@pytest.mark.parametrize('key', dr.ATT_CASES, ids=str)
def test_fp32_evaluation_passes_the_attention_judge(key):
    c = dr.att_case(*key)
    want = dr.tcn_attention_step_ref(*dr.att_args(c))
    tols = dr.att_tolerance(c, want)
    got = dr.tcn_attention_step_ref(*dr.att_args(c), dtype=torch.float32, tanh_form='exp')
    print('%s fp32 distance att %.3g ctx %.3g  tolerance %.3g %.3g' % (key, tols[2], tols[3], tols[0], tols[1]))
    assert dr.judge_att_step(c, got[0], got[1], want, tols) == []
    assert not torch.isnan(want[0]).any()
    if c['sat']:
        assert tols[0] < 1e-4


@pytest.mark.parametrize('shape', dr.GRU_SHAPES, ids=str)
def test_fp32_evaluation_passes_the_gru_judge(shape):
    c = dr.gru_case(shape)
    want = dr.att_gru_step_ref(*dr.gru_args(c), c['beam'])
    tols = dr.gru_tolerance(c, want)
    got = dr.att_gru_step_ref(*dr.gru_args(c), c['beam'], dtype=torch.float32, tanh_form='exp')
    print('%s fp32 distance att %.3g states %.3g  tolerance %.3g %.3g' % (shape, tols[2], tols[3], tols[0], tols[1]))
    assert dr.judge_gru_step(c, got[0], got[1], want, tols) == []
    assert max(tols[:2]) < 1e-4


def _close(a, b, what):
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= 1e-10 * max(scale, 1.0), (what, err, scale)


@pytest.mark.parametrize('T,B,beam,A,E', [(1, 1, 1, 4, 4), (31, 2, 3, 8, 20), (70, 3, 4, 16, 12)])
def test_attention_referee_is_the_module_in_double(T, B, beam, A, E):
    from att_speech.modules.tcn import LocalAttention
    torch.manual_seed(T)
    D, hyps = 10, B * beam
    attn = LocalAttention(E, D, A, temperature=1.25).double()
    with torch.no_grad():
        attn.hidden_to_score.weight.normal_()
    enc = torch.randn(T, B, E, dtype=F64)
    lens = torch.tensor([T, 1, max(1, T // 2)][:B])
    lm_state = torch.randn(hyps, D, dtype=F64)
    prev = torch.softmax(torch.randn(hyps, T, dtype=F64), 1)
    parent = (torch.arange(hyps) // beam) * beam + torch.randint(0, beam, (hyps,))
    with torch.no_grad():
        per_hyp = enc.repeat_interleave(beam, dim=1)
        att_state, _ = attn.init_attention(per_hyp, lens.repeat_interleave(beam))
        att_state = (att_state[0], att_state[1].double())
        _, att = attn(att_state, lm_state, prev.t()[:, parent])
        ctx = torch.bmm(att.t().unsqueeze(1), per_hyp.transpose(0, 1)).squeeze(1)
        got = dr.tcn_attention_step_ref(
            attn.encoded_to_hidden(enc), enc, lens, attn.lm_to_kernel(lm_state).view(hyps, A, 32),
            attn.lm_to_global(lm_state), attn.hidden_to_score.weight.reshape(-1),
            float(attn.hidden_to_score.bias), attn.temperature, prev, parent, beam)
    _close(got[0], att.t(), 'att')
    _close(got[1], ctx, 'context')


@pytest.mark.parametrize('T,NU,beam,H,E', [(1, 1, 1, 4, 4), (33, 2, 3, 12, 36), (50, 3, 4, 16, 8)])
def test_gru_referee_is_the_module_in_double(T, NU, beam, H, E):
    from att_speech.modules.decoders.attention_decoder import AttentionDecoderRNN
    torch.manual_seed(T)
    B = NU * beam
    dec = AttentionDecoderRNN({'features': torch.zeros(T, NU, E)}, 7, 1, H, 0.0).double().eval()
    with torch.no_grad():
        dec.attn.hidden_to_score.weight.normal_()
    enc = torch.randn(T, NU, E, dtype=F64)
    lens = torch.tensor([T, max(1, T // 3), max(1, T - 1)][:NU])
    h0 = torch.randn(B, H, dtype=F64)
    emb = torch.randn(B, H, dtype=F64)
    with torch.no_grad():
        per_hyp = enc.repeat_interleave(beam, dim=1)
        att_state, first = dec.attn.init_attention(per_hyp, lens.repeat_interleave(beam))
        att_state = (att_state[0], att_state[1].double())
        att, output, _ = dec._step(per_hyp, att_state, first.double(), emb, h0[None])
        rnn = dec.rnn
        args = (dec.attn.encoded_to_hidden(enc), enc, lens,
                torch.nn.functional.linear(emb, rnn.weight_ih_l0[:, :H], rnn.bias_ih_l0),
                rnn.weight_ih_l0[:, H:], rnn.weight_hh_l0, rnn.bias_hh_l0,
                dec.attn.rec_state_to_hidden.weight, dec.attn.hidden_to_score.weight.reshape(-1),
                dec.attn.hidden_to_score.bias, h0)
        got = dr.att_gru_step_ref(*args, beam)
        _close(got[0], att.t(), 'att')
        _close(got[1], output[0], 'states')
        # clamp_len: a length of 0 or above T' is T'
        full = dr.att_gru_step_ref(*(args[:2] + (torch.full((NU,), T),) + args[3:]), beam)
        for odd in (0, T + 1, -3):
            alt = dr.att_gru_step_ref(*(args[:2] + (torch.full((NU,), odd),) + args[3:]), beam)
            assert torch.equal(alt[0], full[0]) and torch.equal(alt[1], full[1])


# ---------------------------------------------------------------- the host guard of the LDS limit

def test_native_decode_is_refused_beyond_the_attention_steps_frames():
    from att_speech.modules.tcn import AttentionDecoderTCN
    dec = AttentionDecoderTCN({'features': torch.zeros(4, 1, 8)}, 9, tcn_hidden_size=8,
                              att_hidden_size=4, dropout_p=0.0, beam_size=2).eval()
    fake = lambda T: types.SimpleNamespace(is_cuda=True, dtype=torch.float32, size=lambda d: (T, 1, 8)[d])  # noqa: E731
    assert dec._native_decode_ok(fake(334)) and dec._native_decode_ok(fake(dr.ATT_STEP_MAX_FRAMES))
    assert not dec._native_decode_ok(fake(dr.ATT_STEP_MAX_FRAMES + 1))
    assert (32 - 1 + 2 * dr.ATT_STEP_MAX_FRAMES + 32) * 4 <= 64 * 1024 < (32 - 1 + 2 * (dr.ATT_STEP_MAX_FRAMES + 1) + 32) * 4
