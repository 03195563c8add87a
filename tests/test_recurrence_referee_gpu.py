"""csrc/lstm.hip and csrc/gru.hip judged step by step by the fp64 referees of
tests/recurrence_referee.py (proved on the CPU in tests/test_recurrence_referee.py).

Every case runs the forward kernel, referees every frame teacher-forced (the recurrent operand
is the kernel's own y_bf16 / csave / y of the neighbouring frame), runs the backward kernel on
the kernel's own saved tensors and referees that, then once more on synthetic saved tensors
(recurrence_referee.synthetic_saved).  The rule is per element: a bf16 output must lie between
bf16_round_down(want - d) and bf16_round_up(want + d), an fp32 output within d, d derived in the
referee.  Besides: padding frames of y, dgates, dgx, dhn are exact zeros, y_bf16 is bf16(y) between
two zero frames, nothing is NaN, garbage on padding frames of gx and dy changes nothing, and
lstm_check_errors() is clean.  The matrix (recurrence_referee.CASES) holds every built hidden size
of both recurrences with each kind of lens, B = 1 ... 900, T = 1, 2, 23, 40, 334, gx as fp32 and
bf16, both dy forms, persistent and per-step launches, the base, saturated and quiet draws, and
the fused input projection at F = H."""
import os

import pytest
import torch

import recurrence_referee as rr

pytestmark = pytest.mark.gpu


def _seed(c):
    return c['T'] * 1009 + c['B'] * 31 + c['H']


def _cpu(*ts):
    return [t.cpu() for t in ts]


@pytest.mark.parametrize('c', rr.CASES, ids=rr.case_id)
def test_recurrence_is_refereed_step_by_step(c):
    from att_speech import _native
    dev = torch.device('cuda:0')
    rnn, T, B, H = c['rnn'], c['T'], c['B'], c['H']
    inp = rr.make_inputs(rnn, T, B, H, c['kind'], _seed(c), c['gx_scale'], c['dy_shared'], c['w_scale'])
    lens, whh, whhT, dy = inp['lens'], inp['whh'], inp['whhT'], inp['dy']
    gx = inp['gx'].to(torch.bfloat16) if c['gx_bf16'] else inp['gx']
    lens_d = lens.to(dev, torch.int32)
    gx_mag = K = None
    os.environ['ASR_LSTM_PERSIST'] = '1' if c['persist'] else '0'
    try:
        if c['fused']:
            assert _native.lstm_fused_supported(B, H)
            x, wih, gx, gx_mag = rr.fused_inputs(T, B, H, c['kind'], _seed(c))
            K = 2 * H
            fw = _native.lstm_bidir_fwd_fused(x.to(dev), wih.to(dev), whh.to(dev), lens_d)
        elif rnn == 'lstm':
            fw = _native.lstm_bidir_fwd(gx.to(dev), whh.to(dev), lens_d)
        else:
            assert _native.gru_supported(B, H)
            fw = _native.gru_bidir_fwd(gx.to(dev), whh.to(dev), lens_d)
        syn_gates, syn_other = rr.synthetic_saved(rnn, T, B, H, lens, _seed(c) + 1)
        if rnn == 'lstm':
            y, ybf, gates, csave = fw
            bw = (_native.lstm_bidir_bwd(dy.to(dev), whhT.to(dev), lens_d, gates, csave),)
            bw_syn = (_native.lstm_bidir_bwd(dy.to(dev), whhT.to(dev), lens_d, syn_gates.to(dev), syn_other.to(dev)),)
        else:
            y, ybf, gates = fw
            bw = _native.gru_bidir_bwd(dy.to(dev), whhT.to(dev), lens_d, gates, y)
            bw_syn = _native.gru_bidir_bwd(dy.to(dev), whhT.to(dev), lens_d, syn_gates.to(dev), syn_other.to(dev))
        torch.cuda.synchronize()
    finally:
        os.environ.pop('ASR_LSTM_PERSIST', None)
    _native.lstm_check_errors()
    fw, bw, bw_syn = _cpu(*fw), _cpu(*bw), _cpu(*bw_syn)

    vf, vb, vs = rr.Verdict(), rr.Verdict(), rr.Verdict()
    if rnn == 'lstm':
        y, ybf, gates, csave = fw
        want = rr.lstm_forward(gx, whh, lens, forced=(ybf, csave), gx_mag=gx_mag, K=K)
        rr.judge_lstm_forward(vf, want, y, ybf, gates, csave, lens)
        want = rr.lstm_backward(dy, c['dy_shared'], whhT, lens, gates, csave, forced=bw[0])
        rr.judge_backward(vb, want, {'dgates': bw[0]}, lens, H)
        want = rr.lstm_backward(dy, c['dy_shared'], whhT, lens, syn_gates, syn_other, forced=bw_syn[0])
        rr.judge_backward(vs, want, {'dgates': bw_syn[0]}, lens, H)
    else:
        y, ybf, gates = fw
        want = rr.gru_forward(gx, whh, lens, forced=(ybf, y))
        rr.judge_gru_forward(vf, want, y, ybf, gates, lens)
        want = rr.gru_backward(dy, c['dy_shared'], whhT, lens, gates, y, forced=bw)
        rr.judge_backward(vb, want, {'dgx': bw[0], 'dhn': bw[1]}, lens, H)
        want = rr.gru_backward(dy, c['dy_shared'], whhT, lens, syn_gates, syn_other, forced=bw_syn)
        rr.judge_backward(vs, want, {'dgx': bw_syn[0], 'dhn': bw_syn[1]}, lens, H)
    print('REFEREE %s H=%d max ulp error: forward %.3f backward %.3f synthetic %.3f (checked %d)' % (
        rnn, H, vf.max_ulp, vb.max_ulp, vs.max_ulp, vf.checked + vb.checked + vs.checked))
    assert vf.checked and vb.checked and vs.checked
    assert vf.count == 0, 'forward: ' + vf.report()
    assert vb.count == 0, 'backward: ' + vb.report()
    assert vs.count == 0, 'backward on synthetic saved tensors: ' + vs.report()
