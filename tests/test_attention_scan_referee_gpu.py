"""The attention training scans of csrc/tcn_train.hip and csrc/att_gru.hip, one launch at a time
through the C ABI (asr_tcn_attention_scan_fwd_f32 / _bwd_f32, asr_att_gru_scan_fwd_f32 / _bwd_f32)
on POISONed outputs, judged by the fp64 referee of tests/attention_scan_referee.py (proved on the
CPU by tests/test_attention_scan_referee.py, which also shows that this matrix rejects every
one-term mutant).  The forward is judged teacher-forced on its own alignments / states; the
backward is fed the kernel's own forward outputs.  Nothing here is fitted to what the kernels
return; profiles/attention_scan_referee.md holds the measured shares of the bounds."""
import pytest
import torch

import attention_scan_referee as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_cache = {}
_failed = []


def native():
    from att_speech import _native
    return _native


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def poison(*shape):
    return torch.full(shape, ar.POISON, dtype=torch.float32, device=DEV)


def launch_tcn(c):
    N = native()
    lib, p, st = N.lib(), N._p, N._stream()
    s = c['spec']
    T, B, L, A = (s[k] for k in 'TBLA')
    d = {k: dev(c[k]) for k in ('eproj', 'filt', 'glob', 'a0', 'w_score', 'b_score', 'lens', 'd_att')}
    att = poison(L, B, T)
    N.check(lib.asr_tcn_attention_scan_fwd_f32(
        p(d['eproj']), p(d['filt']), p(d['glob']), p(d['a0']), p(d['w_score']), p(d['b_score']),
        float(c['temperature']), p(d['lens']), T, B, L, A, ar.KF, p(att), st), 'asr_tcn_attention_scan_fwd_f32')
    torch.cuda.synchronize()
    out = dict(d_eproj=poison(T, B, A), d_filt=poison(L, B, A * ar.KF), d_glob=poison(L, B, A),
               d_a0=poison(T, B), d_wb=poison(B, A + 1))
    N.check(lib.asr_tcn_attention_scan_bwd_f32(
        p(d['eproj']), p(d['filt']), p(d['glob']), p(d['a0']), p(d['w_score']), float(c['temperature']),
        p(d['lens']), p(att), p(d['d_att']), T, B, L, A, ar.KF, p(out['d_eproj']), p(out['d_filt']),
        p(out['d_glob']), p(out['d_a0']), p(out['d_wb']), st), 'asr_tcn_attention_scan_bwd_f32')
    torch.cuda.synchronize()
    return dict(att=att.cpu()), {k: v.cpu() for k, v in out.items()}


def launch_gru(c):
    N = native()
    lib, p, st = N.lib(), N._p, N._stream()
    s = c['spec']
    T, B, L, A, E, H = (s[k] for k in 'TBLAEH')
    d = {k: dev(c[k]) for k in ar.GRU_FWD_ARGS + ('d_att', 'd_states')}
    f = dict(att=poison(L, B, T), states=poison(L, B, H), contexts=poison(L, B, E), gates=poison(L, B, 4 * H),
             rec=poison(L, B, A))
    N.check(lib.asr_att_gru_scan_fwd_f32(
        p(d['eproj']), p(d['encoded']), p(d['lens']), p(d['gx_emb']), p(d['w_ic']), p(d['w_hh']), p(d['b_hh']),
        p(d['w_rec']), p(d['w_score']), p(d['b_score']), p(d['h0']), T, B, 1, L, A, E, H, p(f['att']),
        p(f['states']), p(f['contexts']), p(f['gates']), p(f['rec']), st), 'asr_att_gru_scan_fwd_f32')
    torch.cuda.synchronize()
    tr = {k: d[k].t().contiguous() for k in ('w_ic', 'w_hh', 'w_rec')}
    out = dict(d_eproj=dev(c['d_eproj_prefill']), d_gates=poison(L, B, 4 * H), d_contexts=poison(L, B, E),
               d_rec=poison(L, B, A), d_w_score=poison(B, A), d_h0=poison(B, H))
    N.check(lib.asr_att_gru_scan_bwd_f32(
        p(d['eproj']), p(d['encoded']), p(d['lens']), p(tr['w_ic']), p(tr['w_hh']), p(tr['w_rec']),
        p(d['w_score']), p(d['h0']), p(f['att']), p(f['states']), p(f['gates']), p(f['rec']), p(d['d_att']),
        p(d['d_states']), T, B, L, A, E, H, p(out['d_eproj']), p(out['d_gates']), p(out['d_contexts']),
        p(out['d_rec']), p(out['d_w_score']), p(out['d_h0']), st), 'asr_att_gru_scan_bwd_f32')
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in f.items()}, {k: v.cpu() for k, v in out.items()}


def launched(name):
    """the case, and the outputs of its two launches (made once); after a launch that failed as a
    launch nothing more is sent to the device"""
    assert not _failed, 'an earlier launch failed: %s' % _failed[0]
    if name not in _cache:
        c = ar.build(name)
        try:
            _cache[name] = (c,) + (launch_tcn if c['spec']['kind'] == 'tcn' else launch_gru)(c)
        except Exception as e:
            _failed.append('%s: %r' % (name, e))
            raise
    return _cache[name]


def _report(name, op, stats):
    for k in sorted(k for k in stats if not k.endswith(':share')):
        print('MEASURED %s %s %s error %.4g share of the bound %.3f' % (name, op, k, stats[k], stats[k + ':share']))


@pytest.mark.parametrize('name', ar.cases())
def test_forward_launch_against_referee(name):
    c, fwd, _ = launched(name)
    for k, v in fwd.items():
        assert not bool((v == ar.POISON).any()), '%s keeps the POISON' % k
    want, tol = ar.referee(c, 'fwd', fwd['att' if c['spec']['kind'] == 'tcn' else 'states'])
    stats = {}
    bad = ar.judge(c, 'fwd', fwd, want, tol, stats)
    _report(name, 'fwd', stats)
    assert not bad, bad


@pytest.mark.parametrize('name', ar.cases())
def test_backward_launch_against_referee(name):
    c, fwd, bwd = launched(name)
    want, tol = ar.referee(c, 'bwd', fwd, bwd)
    stats = {}
    bad = ar.judge(c, 'bwd', bwd, want, tol, stats)
    _report(name, 'bwd', stats)
    assert not bad, bad


# ---------------------------------------------------------------- gates: a refusal launches nothing

def _tcn_codes(N, buf, out, T=10, B=2, L=3, A=8, Kf=32):
    lib, p, st = N.lib(), N._p, N._stream()
    i, o = p(buf), p(out)
    return (lib.asr_tcn_attention_scan_fwd_f32(i, i, i, i, i, i, 1.25, i, T, B, L, A, Kf, o, st),
            lib.asr_tcn_attention_scan_bwd_f32(i, i, i, i, i, 1.25, i, i, i, T, B, L, A, Kf, o, o, o, o, o, st))


def _gru_codes(N, buf, out, T=10, B=6, beam=1, L=3, A=8, E=8, H=8):
    lib, p, st = N.lib(), N._p, N._stream()
    i, o = p(buf), p(out)
    fwd = lib.asr_att_gru_scan_fwd_f32(i, i, i, i, i, i, i, i, i, i, i, T, B, beam, L, A, E, H, o, o, o, o, o, st)
    if beam != 1:                       # (the backward has no beam: it would take these shapes)
        return fwd, None
    bwd = lib.asr_att_gru_scan_bwd_f32(i, i, i, i, i, i, i, i, i, i, i, i, i, i, T, B, L, A, E, H, o, o, o, o, o, o, st)
    return fwd, bwd


def test_gates_refuse_and_leave_the_poison():
    N = native()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)     # (lens read as int32 zeros)
    out = poison(1 << 16)
    U, INV = N.ASR_EUNSUPPORTED, N.ASR_EINVAL
    for kw in (dict(Kf=31), dict(Kf=33), dict(A=257), dict(T=4097)):
        assert _tcn_codes(N, buf, out, **kw) == (U, U), kw
    for kw in (dict(A=6), dict(E=516), dict(H=324), dict(T=4097), dict(A=324), dict(E=6), dict(H=6)):
        assert _gru_codes(N, buf, out, **kw) == (U, U), kw
    assert _gru_codes(N, buf, out, B=6, beam=4) == (INV, None)      # the beam divides the hypotheses
    for kw in (dict(T=0), dict(B=0), dict(L=0), dict(A=0)):
        assert _tcn_codes(N, buf, out, **kw) == (INV, INV), kw
        assert _gru_codes(N, buf, out, **kw) == (INV, INV), kw
    torch.cuda.synchronize()
    assert bool((out == ar.POISON).all())


# ---------------------------------------------------------------- the wrappers' shape contract

def test_tcn_wrappers_refuse_inconsistent_operands():
    """every wrong operand is LARGER than the consistent one: nothing is read out of bounds even by
    a wrapper that does not look"""
    N = native()
    T, B, L, A = 20, 2, 3, 8
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    ok = dict(eproj=z(T, B, A), filt=z(L, B, A * ar.KF), glob=z(L, B, A), a0=z(T, B), w_score=z(A),
              b_score=z(1), enc_lens=torch.full((B,), T, dtype=torch.int32, device=DEV), temperature=1.0)
    att = N.tcn_attention_scan_fwd(**ok)
    assert tuple(att.shape) == (L, B, T)
    bw = {k: v for k, v in ok.items() if k != 'b_score'}
    bw.update(att=att, d_att=z(L, B, T))
    assert tuple(N.tcn_attention_scan_bwd(**bw)[1].shape) == (L, B, A * ar.KF)
    wrong = dict(filt=z(L + 1, B, A * ar.KF), glob=z(L, B, A + 1), a0=z(T + 1, B), w_score=z(A + 1),
                 enc_lens=torch.full((B + 1,), T, dtype=torch.int32, device=DEV))
    for k, v in wrong.items():
        with pytest.raises(AssertionError):
            N.tcn_attention_scan_fwd(**dict(ok, **{k: v}))
        with pytest.raises(AssertionError):
            N.tcn_attention_scan_bwd(**dict(bw, **{k: v}))
    with pytest.raises(AssertionError):
        N.tcn_attention_scan_fwd(**dict(ok, filt=z(L, B, A * ar.KF + 4)))       # no whole number of taps
    for k, v in dict(att=z(L + 1, B, T), d_att=z(L, B, T + 1)).items():
        with pytest.raises(AssertionError):
            N.tcn_attention_scan_bwd(**dict(bw, **{k: v}))
