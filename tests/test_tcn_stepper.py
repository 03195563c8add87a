"""The label-step driver of the device TCN decode paths (att_speech.modules.tcn._DeviceStepper) on
the CPU: `_native.tcn_attention_step` is replaced by the project's torch referees in fp32
(decode_referee.tcn_attention_step_ref, ff_referee.tcn_attention_step_win_ref under a window), so
what runs is the driver's own part — the per-call operands, TCN.last_step, the filter / global
product, the output MLP and the history roll — in both callers' layouts:

* the searches': `beam` rows per utterance, parents within the utterance, 8 steps;
* the forced scorer's: levels of 1, 2 and 3 rows per utterance, `parent` indexing the previous
  level's rows, so that the previous alignments have fewer rows than the step puts out.

Every step is held against the host `enc_step` (full TCN, LocalAttention.forward) on the same
parents and labels, within the tolerances of the CPU checks of test_tcn_beam.py / test_tcn_ff.py:
alignments 1e-5, logits 2e-4 absolute (logits of magnitude ~45 here)."""
import numpy as np
import pytest
import torch

import decode_referee as dr
import ff_referee as fr

T, B, E, S, BEAM, STEPS = 40, 2, 16, 6, 3, 8
LENS = (40, 23)
KW = dict(tcn_hidden_size=24, att_hidden_size=8, dropout_p=0.0, kernel_size=3, dilation_sizes=[1, 2],
          beam_size=BEAM, length_normalization=0.6, attention_temperature=1.25, tcn_layers_per_block=2)
ATT_TOL, LOGITS_TOL = 1e-5, 2e-4


def referee_step(*args, **kw):
    """the signature of _native.tcn_attention_step, answered by the torch referees in fp32"""
    window = kw.pop('window', None)
    assert not kw
    if window is None:
        return dr.tcn_attention_step_ref(*args, dtype=torch.float32)
    return fr.tcn_attention_step_win_ref(*args, window, dtype=torch.float32)


def fixture(window):
    from att_speech.modules.tcn import AttentionDecoderTCN
    gen = torch.Generator().manual_seed(1407)
    dec = AttentionDecoderTCN({'features': torch.zeros(T, B, E)}, S, att_force_forward=window, **KW).eval()
    with torch.no_grad():
        for prm in dec.parameters():
            prm.add_(torch.randn(prm.shape, generator=gen) * 0.3)
    return dec, torch.randn(T, B, E, generator=gen), gen


def close(got_logits, got_att, want_logits, want_att, where):
    """want_att [T, rows] as the host keeps it"""
    print('%s: attention distance %.3g, logits distance %.3g (scale %.3g)' % (
        where, float((got_att - want_att.t()).abs().max()), float((got_logits - want_logits).abs().max()),
        float(want_logits.abs().max())))
    np.testing.assert_allclose(got_att.numpy(), want_att.t().numpy(), rtol=0, atol=ATT_TOL, err_msg=str(where))
    np.testing.assert_allclose(got_logits.numpy(), want_logits.numpy(), rtol=0, atol=LOGITS_TOL,
                               err_msg=str(where))


@pytest.mark.parametrize('window', [None, (-2, 6)], ids=str)
def test_stepper_follows_enc_step_in_both_layouts(window, monkeypatch):
    from att_speech import _native
    from att_speech.modules.tcn import _DeviceStepper
    monkeypatch.setattr(_native, 'tcn_attention_step', referee_step)
    dec, enc, gen = fixture(window)
    lens = torch.tensor(LENS, dtype=torch.int32)
    draw = lambda hi, n: torch.randint(0, hi, (n,), generator=gen)  # noqa: E731
    with torch.no_grad():
        stepper = _DeviceStepper(dec, enc, lens)
        assert stepper.window == window and stepper.first.shape == (T, B)

        # ---- the searches' layout: BEAM rows per utterance
        hyps = B * BEAM
        state = dec.enc_initial_state(enc, lens, BEAM, B)
        np.testing.assert_array_equal(state['att_weights'].numpy(),
                                      stepper.first.repeat_interleave(BEAM, dim=1).numpy())
        att = stepper.first.t().repeat_interleave(BEAM, dim=0).contiguous()
        history, parent = stepper.empty_history(hyps), None
        assert history.shape == state['inputs'].shape
        peaked = 0
        for s in range(STEPS):
            peaked += int(((att if parent is None else att[parent.long()]).max(1)[0] >= 0.1).sum())
            host_history = state['inputs']
            want_logits, state = dec.enc_step(**state)
            logits, att = stepper.step(history, att, parent, BEAM)
            assert logits.shape == (hyps, S + 1) and att.shape == (hyps, T)
            close(logits, att, want_logits[0], state['att_weights'], ('search', s))
            parent = (torch.arange(hyps) // BEAM * BEAM + draw(BEAM, hyps)).to(torch.int32)
            labels = draw(S, hyps).to(torch.int32)
            history = stepper.roll(history, parent, labels)
            state['att_weights'] = state['att_weights'][:, parent.long()]
            state['inputs'] = torch.cat((host_history[1:, parent.long()], dec.embedding(labels.long())[None]))
            np.testing.assert_array_equal(history.numpy(), state['inputs'].numpy())
        assert peaked > 0           # previous alignments sharp enough for the window to act on

        # ---- the scorer's layout: levels of 1, 2, 3 rows per utterance
        history, att = stepper.empty_history(B), stepper.first.t().contiguous()
        host_history, host_att = history.clone(), stepper.first.clone()                 # [., rows, D], [T, rows]
        width_prev = 1
        for l, width in enumerate((1, 2, 3)):
            rows = B * width
            utt = torch.arange(rows) // width
            parent = utt * width_prev + (draw(width_prev, rows) if l else 0)
            if l:
                labels = draw(S, rows)
                history = stepper.roll(history, parent, labels)
                host_history = torch.cat((host_history[1:, parent], dec.embedding(labels)[None]))
            logits, att = stepper.step(history, att, parent.to(torch.int32), width)
            assert logits.shape == (rows, S + 1) and att.shape == (rows, T)
            want_logits, want_att = [], []
            for r in range(rows):                       # the host step, one row at a time
                u, p = int(utt[r]), int(parent[r])
                att_state, _ = dec.attn.init_attention(enc[:, u:u + 1], lens[u:u + 1])
                lg, st = dec.enc_step(host_history[:, r:r + 1], enc[:, u:u + 1], att_state, host_att[:, p:p + 1])
                want_logits.append(lg[0])
                want_att.append(st['att_weights'])
            host_att = torch.cat(want_att, 1)
            close(logits, att, torch.cat(want_logits), host_att, ('scorer', l, width))
            width_prev = width
