"""asr_tcn_attention_step_win_f32 and the device searches it opens to models with
`att_force_forward`, on the MI355X:

* single launches against the fp64 referee of tests/ff_referee.py (proved on the CPU by
  tests/test_tcn_ff.py: it is the host mirror in double, the matrix reaches every kind of row,
  each of six mutants is caught).  Alignment and context are held to 4x the distance of the fp32
  evaluation of the same formula from fp64 plus the tanh term (decode_referee.att_tolerance's
  rule); rows sum to 1 within 1e-5; every frame the referee puts off the support is exactly 0;
* tests/golden/tcn_beam_ff.npz, the reference's own decode under the window (-2, 6), through
  DeviceBeamSearch for beam 1 and beam 3;
* the recipe's dimensions and its window (-10, 50) against the host mirror on the CPU;
* the LM-fused search of a batch (DeviceBeamSearchLM) against the host BeamSearchLM decode of
  each utterance, every decision of the device's own trajectory above the margin floor;
* ASR_TCN_FF_NATIVE=0 gives the host classes and the same labels."""
import os
import warnings

import numpy as np
import pytest
import torch

import decode_referee as dr
import ff_referee as fr
import lm_beam_referee as lr
from conftest import golden
from ff_referee import as_lists, check_fixture_decode, fixture_decoder, want_of

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def native():
    from att_speech import _native
    return _native


# ---------------------------------------------------------------- single launches

def test_every_kind_of_row_occurs_in_the_launches_below():
    seen = fr.kinds_seen(fr.FF_CASES)
    assert set(fr.FF_KINDS) <= set(seen), set(fr.FF_KINDS) - set(seen)
    assert any(w == (-10, 50) for _, _, w in seen['straddles_256'])        # peak at 250
    assert any(w == (1, 6) for _, _, w in seen['behind_len'])               # peak at len - 1


@pytest.mark.parametrize('key', fr.FF_CASES + fr.FF_LENGTH_CASES, ids=str)
def test_windowed_attention_step(key):
    c, want, tols = want_of(key)
    args = fr.ff_args(c, DEV)
    att, ctx = native().tcn_attention_step(*args[:-1], window=args[-1])
    att, ctx = att.cpu(), ctx.cpu()
    print('%s fp32 distance att %.3g ctx %.3g  kernel error att %.3g ctx %.3g  tolerance %.3g %.3g' % (
        key, tols[2], tols[3], float((att.double() - want[0]).abs().max()),
        float((ctx.double() - want[1]).abs().max()), tols[0], tols[1]))
    assert not torch.isnan(att).any() and not torch.isnan(ctx).any()
    assert fr.judge_ff_step(c, att, ctx, want, tols) == []


def test_a_window_that_never_bites_is_the_plain_step():
    """a window wider than the row on both sides masks nothing: the same weights as
    asr_tcn_attention_step_f32 on the frames below len, within rounding of the score sum"""
    c = fr.ff_case((334, 3, 10, 64, 320), 1, (-10, 50))
    args = dr.att_args(c, DEV)
    plain_att, plain_ctx = native().tcn_attention_step(*args)
    att, ctx = native().tcn_attention_step(*args, window=(-400, 400))
    torch.testing.assert_close(att, plain_att, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(ctx, plain_ctx, rtol=1e-4, atol=1e-5)


def test_refused_windows_launch_nothing():
    c = fr.ff_case((9, 2, 3, 8, 20), 0, (-2, 6))
    args = dr.att_args(c, DEV)
    for window in ((3, 3), (-5, 0), (4, 2)):
        with pytest.raises(NotImplementedError):
            native().tcn_attention_step(*args, window=window)
    with pytest.raises(TypeError):
        native().tcn_attention_step(*args, window=(-2.5, 6))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the reference's decode

@pytest.mark.parametrize('beam', [1, 3])
def test_fixture_decodes_on_the_device(beam):
    from att_speech.modules.beam_search import DeviceBeamSearch
    g = golden('tcn_beam_ff.npz')
    dec, enc = fixture_decoder(g, DEV)
    dec.beam_size = beam
    assert dec._native_decode_ok(enc)
    with torch.no_grad():
        res = dec.decode(enc, torch.from_numpy(g['lens']), return_attention=True)
        plain = dec.decode(enc, torch.from_numpy(g['lens']))          # flag polled every 8 steps
    assert isinstance(res['beam_search'], DeviceBeamSearch)
    assert isinstance(plain['beam_search'], DeviceBeamSearch)
    check_fixture_decode(g, res, beam, att_tol=2e-4, score_tol=2e-4)
    assert as_lists(plain['decoded']) == as_lists(res['decoded'])


# ---------------------------------------------------------------- recipe dimensions

def _recipe_decoder():
    """lattice_decoding/tcn.yaml dimensions with the readme's window.  Seed 4258 and the factor 20
    on hidden_to_score were picked on the CPU among seeds 4242..4289: the host mirror alone has
    the window active on every (step, hypothesis) row (the score vector starts at zero, so
    without the factor every alignment is uniform over the window and diffuse), decodes 18 to 27
    labels per utterance in 28 steps, and its smallest decision margin (kept against dropped and
    neighbouring kept candidates, EOS against the best class) is 1.2e-4."""
    from att_speech.modules.tcn import AttentionDecoderTCN
    torch.manual_seed(4258)
    S, T, B, E = 49, 90, 5, 320
    kw = dict(tcn_hidden_size=384, att_hidden_size=64, dropout_p=0.0, kernel_size=3,
              dilation_sizes=[1, 2], beam_size=10, length_normalization=0.6,
              attention_temperature=1.25, tcn_layers_per_block=2,
              att_force_forward=(-10, 50), learnable_initial_attention=False)
    dec = AttentionDecoderTCN({'features': torch.zeros(T, B, E)}, S, **kw).eval()
    with torch.no_grad():
        for prm in dec.parameters():
            prm.add_(torch.randn_like(prm) * 0.05)
        dec.attn.hidden_to_score.weight.mul_(20.0)
        dec.output_to_logits.bias[S] += 1.5            # EOS competitive: hypotheses finish
    enc = torch.randn(T, B, E)
    lens = torch.tensor([90, 81, 77, 60, 41])
    dec.TRANSCRIPTION_LEN_GUARD = 40
    return dec, enc, lens


def test_recipe_dims_under_the_recipe_window_match_the_cpu_mirror():
    from att_speech.modules.beam_search import BeamSearch, DeviceBeamSearch
    dec, enc, lens = _recipe_decoder()
    with torch.no_grad():
        want = dec.decode(enc, lens, return_attention=True)
        peaks = torch.stack(want['attweights'][:-1]).max(1)[0]       # [steps, hyp]
        active = float((peaks >= 0.1).float().mean())
        print('host mirror: %d steps, window active on %.0f %% of the rows' % (peaks.shape[0], 100 * active))
        assert active >= 0.5
        dev = torch.device(DEV)
        dec_g = dec.to(dev)
        assert dec_g._native_decode_ok(enc.to(dev))
        got = dec_g.decode(enc.to(dev), lens)
    assert isinstance(want['beam_search'], BeamSearch)
    assert isinstance(got['beam_search'], DeviceBeamSearch)
    assert as_lists(got['decoded']) == as_lists(want['decoded'])
    assert any(len(d) > 0 for d in as_lists(want['decoded']))
    wb, gb = want['beam_search'], got['beam_search']
    assert gb.finished_count == wb.finished_count
    np.testing.assert_array_equal(gb.estimations.cpu().numpy(), wb.estimations.numpy())
    np.testing.assert_allclose(gb.scores.cpu().numpy(), wb.scores.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(np.array(got['decoded_scores']['acoustic']),
                               np.array(want['decoded_scores']['acoustic']), rtol=2e-4)


# ---------------------------------------------------------------- LM-fused decode

VOCAB = ['<pad>', '<unk>', ' ', 'a', 'b', 'c']
LM_WINDOW = (-2, 6)


def _lm_decoder(lm, seed, **kw):
    """the decoder of test_lm_beam_gpu.py under a window, the first alignment a one-hot"""
    from att_speech.modules.tcn import AttentionDecoderTCN
    torch.manual_seed(seed)
    args = dict(tcn_hidden_size=32, att_hidden_size=8, dropout_p=0.0, kernel_size=3, dilation_sizes=[1, 2],
                beam_size=3, length_normalization=0.6, vocabulary=VOCAB, lm_file=lm, lm_weight=0.5,
                coverage_weight=0.1, coverage_tau=0.1, min_attention_pos=0.3,
                att_force_forward=LM_WINDOW, learnable_initial_attention=False)
    args.update(kw)
    dec = AttentionDecoderTCN({'features': torch.zeros(14, 3, 16)}, 6, **args).eval().to(DEV)
    dec.TRANSCRIPTION_LEN_GUARD = 12
    return dec


def _env(name, value):
    class _Set(object):
        def __enter__(self):
            self.old = os.environ.get(name)
            os.environ[name] = value

        def __exit__(self, *exc):
            if self.old is None:
                del os.environ[name]
            else:
                os.environ[name] = self.old
    return _Set()


def _lm_inputs():
    gen = torch.Generator().manual_seed(5)
    lens = [14, 9, 6]
    enc = torch.randn(14, 3, 16, generator=gen)
    for b, ln in enumerate(lens):
        enc[ln:, b] = 0
    return enc.to(DEV), lens


def test_lm_fused_decode_of_a_batch_under_a_window():
    from att_speech.modules.beam_search import BeamSearchLM, DeviceBeamSearchLM
    # model seed 20: picked on the CPU (host decode per utterance, replayed through lr.RefSearch)
    # for a smallest margin of 0.034 along the whole trajectory among seeds 0..23; asserted below
    # on the device's own logits and alignments.  The window is active on every row (smallest
    # peak 0.17: a one-hot first, then at most 8 frames with a weight).
    dec = _lm_decoder(lr.toy_lm(), seed=20)
    enc, lens = _lm_inputs()
    B, beam, C, T = 3, 3, 7, 14
    assert dec._native_lm_ok(enc) and dec._native_decode_ok(enc)
    with torch.no_grad():
        res = dec.decode(enc, torch.tensor(lens))
        traced = dec.decode(enc, torch.tensor(lens), return_attention=True)
    assert isinstance(res['beam_search'], DeviceBeamSearchLM)
    peaks = torch.stack(traced['attweights'][:-1]).max(1)[0]
    assert float(peaks.min()) >= 0.1                                  # the window was active throughout
    assert int((torch.stack(traced['attweights'][1:]) > 0).sum(1).max()) <= 8
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
    with _env('ASR_LM_BEAM_NATIVE', '0'), torch.no_grad():
        hosts = [dec.decode(enc[:lens[b], b:b + 1].contiguous(), torch.tensor([lens[b]])) for b in range(B)]
    assert all(isinstance(h['beam_search'], BeamSearchLM) for h in hosts)
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


# ---------------------------------------------------------------- the A/B switch

def test_switch_sends_windowed_models_to_the_host_classes():
    from att_speech.modules.beam_search import (BeamSearch, BeamSearchLM, DeviceBeamSearch,
                                                 DeviceBeamSearchLM)
    g = golden('tcn_beam_ff.npz')
    dec, enc = fixture_decoder(g, DEV)
    lens = torch.from_numpy(g['lens'])
    with torch.no_grad():
        on = dec.decode(enc, lens)
        with _env('ASR_TCN_FF_NATIVE', '0'):
            assert not dec._native_decode_ok(enc)
            off = dec.decode(enc, lens)
    assert isinstance(on['beam_search'], DeviceBeamSearch) and isinstance(off['beam_search'], BeamSearch)
    assert as_lists(on['decoded']) == as_lists(off['decoded'])
    # with an LM: the host class takes one utterance per call
    lm_dec = _lm_decoder(lr.toy_lm(), seed=20)
    lm_enc, lm_lens = _lm_inputs()
    one, n = lm_enc[:lm_lens[1], 1:2].contiguous(), torch.tensor([lm_lens[1]])
    with torch.no_grad(), _env('ASR_LM_BEAM_NATIVE', '1'):
        on = lm_dec.decode(one, n)
        with _env('ASR_TCN_FF_NATIVE', '0'):
            off = lm_dec.decode(one, n)
    assert isinstance(on['beam_search'], DeviceBeamSearchLM) and isinstance(off['beam_search'], BeamSearchLM)
    assert as_lists(on['decoded']) == as_lists(off['decoded'])
