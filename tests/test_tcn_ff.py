"""LocalAttention's force_forward window in the TCN decoder, without a GPU:

* the host mirror (modules/tcn.py on the CPU) reproduces tests/golden/tcn_beam_ff.npz, the
  decode of the reference's own tcn.py under `att_force_forward = (-2, 6)` for beam 1 and beam 3
  (make_golden_tcn_ff.py), and the same weights without the window align otherwise;
* tests/ff_referee.py, the fp64 statement of asr_tcn_attention_step_win_f32, is the host mirror
  in double on the cases the GPU test launches, the mirror's fp32 evaluation passes the judge,
  the case matrix reaches every kind of row the kernel has a branch for, and each of the six
  one-term mutants is caught by at least one case;
* the decode gates take the windows the kernel takes and no others; training stays closed;
* the C entry is exported and refuses bad arguments before anything is launched."""
import warnings

import numpy as np
import pytest
import torch

import decode_referee as dr
import ff_referee as fr
from conftest import golden
from ff_referee import check_fixture_decode, fixture_decoder, want_of

warnings.filterwarnings('ignore')

@pytest.mark.parametrize('beam', [1, 3])
def test_host_mirror_reproduces_the_reference_under_the_window(beam):
    g = golden('tcn_beam_ff.npz')
    assert tuple(g['window']) == (-2, 6) and g['lens'].tolist() == [40, 23, 9]
    assert float(g['b%d_margin' % beam]) > dr.MARGIN_FLOOR
    assert float(g['b%d_min_peak' % beam]) >= 0.125          # the window was active on every row
    dec, enc = fixture_decoder(g, 'cpu')
    dec.beam_size = beam
    with torch.no_grad():
        res = dec.decode(enc, torch.from_numpy(g['lens']), return_attention=True)
    check_fixture_decode(g, res, beam, att_tol=1e-5, score_tol=1e-4)
    # an active window leaves at most hi - lo frames with a weight
    att = g['b%d_att' % beam][1:]
    assert int((att > 0).sum(1).max()) <= 8


def test_the_window_bites():
    g = golden('tcn_beam_ff.npz')
    dec, enc = fixture_decoder(g, 'cpu', window=None)
    dec.beam_size = 1
    with torch.no_grad():
        res = dec.decode(enc, torch.from_numpy(g['lens']), return_attention=True)
    free, held = res['attweights'][1].numpy(), g['b1_att'][1]
    assert int((free > 0).sum(0).min()) > 8                  # weight on frames the window forbids
    assert float(np.abs(free - held).max()) > 1e-2


# ---------------------------------------------------------------- the referee

def mirror(c, dtype):
    """LocalAttention.scores + softmax + the context of enc_step on a case's operands: the LM
    state is a one-hot per hypothesis, so the filter / global layers hand out the case's rows"""
    from att_speech.modules.tcn import LocalAttention
    T, B, A = c['eproj'].shape
    beam, hyps, E = c['beam'], B * c['beam'], c['enc'].shape[2]
    attn = LocalAttention(E, hyps, A, temperature=c['temperature'], force_forward=c['window']).to(dtype)
    with torch.no_grad():
        attn.lm_to_kernel.weight.copy_(c['filt'].reshape(hyps, A * fr.KF).t())
        attn.lm_to_kernel.bias.zero_()
        attn.lm_to_global.weight.copy_(c['glob'].t())
        attn.lm_to_global.bias.zero_()
        attn.hidden_to_score.weight.copy_(c['w_score'][None])
        attn.hidden_to_score.bias.fill_(c['b_score'])
        u = torch.arange(hyps) // beam
        pad = attn._padding_scores(c['lens'].long()[u], T, 'cpu').to(dtype)
        src = torch.arange(hyps) if c['parent'] is None else c['parent'].long()
        prev = c['att_prev'].to(dtype)[src].t()
        _, att = attn((c['eproj'].to(dtype)[:, u], pad), torch.eye(hyps, dtype=dtype), prev)
        ctx = torch.bmm(att.t().unsqueeze(1), c['enc'].to(dtype)[:, u].transpose(0, 1)).squeeze(1)
    return att.t(), ctx


@pytest.mark.parametrize('key', fr.FF_CASES + fr.FF_LENGTH_CASES, ids=str)
def test_referee_is_the_host_mirror(key):
    c, want, tols = want_of(key)
    att, ctx = mirror(c, torch.float64)
    for a, b, what in ((want[0], att, 'att'), (want[1], ctx, 'context')):
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        assert err <= 1e-10 * max(scale, 1.0), (what, err, scale)
    assert not torch.isnan(want[0]).any()
    # the mirror in fp32 (torch ops, torch.tanh) and the referee's own fp32 run with the kernels'
    # form of tanh both pass the judge the kernel is held to
    att32, ctx32 = mirror(c, torch.float32)
    print('%s fp32 distance att %.3g ctx %.3g  tolerance %.3g %.3g' % (key, tols[2], tols[3], tols[0], tols[1]))
    assert fr.judge_ff_step(c, att32, ctx32, want, tols) == []
    e32 = fr.tcn_attention_step_win_ref(*fr.ff_args(c), dtype=torch.float32, tanh_form='exp')
    assert fr.judge_ff_step(c, e32[0], e32[1], want, tols) == []


def test_case_matrix_reaches_every_kind_of_row():
    seen = fr.kinds_seen(fr.FF_CASES)
    print({k: len(v) for k, v in sorted(seen.items())})
    assert set(fr.FF_KINDS) <= set(seen), set(fr.FF_KINDS) - set(seen)
    assert {'clipped_to_nothing', 'two_pieces'} <= set(seen)
    # the ones the issue names with their window
    assert any(w == (-10, 50) for _, _, w in seen['straddles_256'])
    assert any(w == (1, 6) for _, _, w in seen['behind_len'])
    # each case with parent null and with a map that is no bijection
    for (shape, draw, window) in fr.FF_CASES:
        c = fr.ff_case(shape, draw, window)
        assert (c['parent'] is None) == (draw == 0)
        if draw == 1 and shape[2] > 1:
            assert len(set(c['parent'].tolist())) < c['parent'].numel()


def test_closed_form_of_the_support_is_the_frames_with_the_fewest_masks():
    """the derivation in csrc/tcn_step.hip, on every row of the matrix and on lengths 0 and > T'"""
    rows = 0
    for key in fr.FF_CASES:
        c = fr.ff_case(*key)
        T = key[0][0]
        for lens in (c['lens'], torch.zeros_like(c['lens']), c['lens'] + T):
            m, info = fr.window_masks(c['att_prev'], c['parent'], lens, c['beam'], c['window'])
            for h in range(m.shape[0]):
                M, P, Q = fr.support_closed_form(info['where'][h], bool(info['active'][h]),
                                                 lens[h // c['beam']], T, c['window'])
                on = torch.zeros(T, dtype=torch.bool)
                on[P[0]:P[1]] = True
                on[Q[0]:Q[1]] = True
                assert M == int(m[h].min()) and torch.equal(on, m[h] == M), (key, h, M, P, Q)
                assert P[1] <= Q[0] or Q[0] == Q[1]
                rows += 1
    assert rows > 1000


def test_length_cases_reach_two_masks_everywhere_and_no_padding():
    most, unpadded = 0, False
    for key in fr.FF_LENGTH_CASES:
        c = fr.ff_case(*key)
        m, info = fr.window_masks(c['att_prev'], c['parent'], c['lens'], c['beam'], c['window'])
        most = max(most, int(m.min(1)[0].max()))
        beyond = (c['lens'].long() > key[0][0]).repeat_interleave(c['beam'])
        unpadded |= bool((beyond & info['active']).any())
    assert most == 2 and unpadded


@pytest.mark.parametrize('mut', fr.FF_MUTANTS)
def test_mutant_is_caught(mut):
    hit = []
    for key in fr.FF_CASES:
        c, want, tols = want_of(key)
        got = fr.tcn_attention_step_win_ref(*fr.ff_args(c), mut=mut)
        if fr.judge_ff_step(c, got[0], got[1], want, tols):
            hit.append(key)
    print('%-24s caught at %2d cases: %s' % (mut, len(hit), hit[:4]))
    assert hit


# ---------------------------------------------------------------- gates

class _FakeCuda(object):
    """Stands in for a CUDA tensor in the gates (shape, dtype, is_cuda only)."""

    def __init__(self, T=50, B=2, dtype=torch.float32):
        self.is_cuda, self.dtype, self._shape = True, dtype, (T, B, 16)
        self.device = torch.device('cpu')       # (only handed to the fake LM)

    def size(self, d):
        return self._shape[d]


class _FakeLm(object):
    """An LM the device search would take, without a device"""
    ilabel = np.array([1, 2, 3])

    def eps_rank(self):
        return [0]

    def device_arrays(self, device):
        return object()

    def input_symbols(self):
        return [(0, '<eps>'), (1, '<spc>'), (2, 'a'), (3, 'b')]


def _decoder(window, lm=False):
    from att_speech.modules.tcn import AttentionDecoderTCN
    dec = AttentionDecoderTCN({'features': torch.zeros(5, 2, 16)}, 7, att_force_forward=window,
                              vocabulary=list('ab cdef'), **fr.FIXTURE_KW)
    if lm:
        dec.lm = _FakeLm()
    return dec.eval()


def test_gates(monkeypatch):
    for name in ('ASR_TCN_NATIVE', 'ASR_TCN_FF_NATIVE', 'ASR_LM_BEAM_NATIVE'):
        monkeypatch.delenv(name, raising=False)
    fake = _FakeCuda()
    for window in ((-10, 50), (-2, 6), [-2, 6]):
        assert _decoder(window)._native_decode_ok(fake)
        with_lm = _decoder(window, lm=True)
        assert with_lm._native_lm_ok(fake) and with_lm._native_decode_ok(fake)
        assert not _decoder(window)._native_decode_ok(torch.zeros(5, 2, 16))      # a CPU tensor
    for window in ((3, 3), (-5, 0), (-2.5, 6), (4, 2), (-2, 6, 1), (True, 6)):
        assert not _decoder(window)._native_decode_ok(fake), window
        with_lm = _decoder(window, lm=True)
        assert not with_lm._native_lm_ok(fake) and not with_lm._native_decode_ok(fake), window
    assert _decoder(None)._native_decode_ok(fake) and _decoder(None, lm=True)._native_lm_ok(fake)
    # the switches are read per call
    monkeypatch.setenv('ASR_TCN_FF_NATIVE', '0')
    assert not _decoder((-2, 6))._native_decode_ok(fake)
    assert not _decoder((-2, 6), lm=True)._native_lm_ok(fake)
    assert _decoder(None)._native_decode_ok(fake)                # models without a window: untouched
    monkeypatch.setenv('ASR_TCN_FF_NATIVE', '1')
    assert _decoder((-2, 6))._native_decode_ok(fake)
    monkeypatch.setenv('ASR_TCN_NATIVE', '0')
    assert not _decoder((-2, 6))._native_decode_ok(fake)
    monkeypatch.delenv('ASR_TCN_NATIVE')
    # an LM-fused single utterance stays on the host unless asked for, window or not
    assert not _decoder((-2, 6), lm=True)._native_lm_ok(_FakeCuda(B=1))
    # rescoring and the graph search keep the host path
    graph = _decoder((-2, 6), lm=True)
    graph.use_graph_search = True
    assert not graph._native_lm_ok(fake)
    # training keeps the per-position loop under a window
    monkeypatch.delenv('ASR_TCN_TRAIN_NATIVE', raising=False)
    assert not _decoder((-2, 6))._native_train_ok(fake)
    assert not _decoder((-10, 50))._native_train_ok(fake)
    assert _decoder(None)._native_train_ok(fake)


# ---------------------------------------------------------------- the C entry

def _call(L, ptr, T=10, B=2, beam=3, A=8, K=32, E=16, lo=-2, hi=6, last=None):
    return L.asr_tcn_attention_step_win_f32(ptr, ptr, ptr, ptr, ptr, ptr, 0.3, 1.25, ptr, None,
                                            T, B, beam, A, K, E, lo, hi, ptr,
                                            ptr if last is None else last, None)


def test_entry_is_exported_and_refuses_before_launching():
    from att_speech import _native
    L = _native.lib()
    assert hasattr(L, 'asr_tcn_attention_step_win_f32')
    assert 'asr_tcn_attention_step_win_f32' in _native._SIGNATURES
    p = 0x1000          # a non-null dummy address: every check must fire before anything is launched
    assert _call(L, None) == _native.ASR_EINVAL
    assert _call(L, p, last=0) == _native.ASR_EINVAL
    for bad in (dict(T=0), dict(B=0), dict(beam=0), dict(A=0), dict(E=0), dict(T=-3)):
        assert _call(L, p, **bad) == _native.ASR_EINVAL
    assert _call(L, p, K=3) == _native.ASR_EUNSUPPORTED
    assert _call(L, p, lo=3, hi=3) == _native.ASR_EUNSUPPORTED
    assert _call(L, p, lo=6, hi=2) == _native.ASR_EUNSUPPORTED
    assert _call(L, p, lo=-5, hi=0) == _native.ASR_EUNSUPPORTED
    assert _call(L, p, lo=-9, hi=-3) == _native.ASR_EUNSUPPORTED
    assert _call(L, p, T=8161) == _native.ASR_EUNSUPPORTED

