"""The BatchNorm2d + Hardtanh kernels of csrc/bnact.hip, one launch at a time through the C ABI
(asr_bn_act_fwd_f32, asr_bn_act_bwd_f32, asr_bn_act_bwd_phase_f32) on POISONed outputs, judged by
the fp64 referee of tests/bn_referee.py (proved on the CPU by tests/test_bn_referee.py, which also
shows that this matrix rejects twelve one-term mutants and reaches every kernel instantiation).
The exact-integer cases are held with torch.equal, everything else to the tolerances derived in
the referee's docstring; nothing here is fitted to what the kernels return.

What this file found, measured on the MI355X with the kernels as they were (see
profiles/bn_referee.md for the figures): the channels-last sums dropped every channel from 256 up
(C = 512 and C = 1024 in training mode: mean 0, invstd 1 / sqrt(eps), zero parameter gradients);
a NaN in x came out as `lo`; the variance, an uncentred difference of fp32 sums, missed the
centred bound at |mean| / std = 64."""
import numpy as np
import pytest
import torch

import bn_referee as br

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = br.cases()
_cache = {}


def native():
    from att_speech import _native
    return _native


def prepared(name):
    if name not in _cache:
        inp = br.build(name)
        op = inp['spec']['op']
        want = br.reference(op, inp)
        tol = None if inp['spec']['kind'] == 'exact' else br.tolerances(op, inp, want)
        _cache[name] = (op, inp, want, tol)
    return _cache[name]


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return None if t is None else t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def poison(n, dtype=torch.float32):
    return torch.full((n,), float(br.POISON), dtype=dtype, device=DEV)


def workspace(N, C, sums=None):
    nbytes = N.lib().asr_bn_act_workspace_bytes(C)
    ws = torch.full((nbytes // 8,), float(br.POISON), dtype=torch.float64, device=DEV)
    if sums is not None:
        ws[:2 * C] = dev(sums)
    return ws, nbytes


def launch_abi(op, inp):
    """one call of the C entry on poisoned outputs -> the outputs as bn_referee.judge takes them"""
    N = native()
    L, p, st = N.lib(), N._p, N._stream()
    s = inp['spec']
    B, C, H, W = shape = tuple(s[k] for k in 'BCHW')
    xl, ol = br.layouts(s)
    xdt = torch.bfloat16 if s['x_bf16'] else torch.float32
    odt = torch.bfloat16 if s['o_bf16'] else torch.float32
    x = dev(br.to_storage(inp['x'], xl), xdt)
    gamma, beta, cb = dev(inp['gamma']), dev(inp['beta']), dev(inp['conv_bias'])
    if op == 'fwd':
        rm, rv = dev(inp['running_mean']), dev(inp['running_var'])
        out, mean, invstd = poison(x.numel(), odt), poison(C), poison(C)
        ws, nbytes = workspace(N, C)
        cs = dev(inp.get('chan_sums'))
        N.check(L.asr_bn_act_fwd_f32(
            p(x), int(s['x_bf16']), p(cb), B, C, H, W, p(gamma), p(beta), p(rm), p(rv), int(s['cl']),
            int(s['training']), float(inp['momentum']), float(inp['eps']), s['lo'], s['hi'], p(out),
            int(s['o_bf16']), int(s['tm']), p(mean), p(invstd), p(cs), p(ws), nbytes, st), 'asr_bn_act_fwd_f32')
        torch.cuda.synchronize()
        return dict(out=br.from_storage(host(out), shape, ol), save_mean=host(mean), save_invstd=host(invstd),
                    running_mean=host(rm), running_var=host(rv))
    dy = dev(br.to_storage(inp['dy'], ol), odt)
    mean, invstd = dev(inp['save_mean']), dev(inp['save_invstd'])
    dx, dgamma, dbeta = poison(x.numel(), xdt), poison(C), poison(C)
    dcb = poison(C) if cb is not None else None                     # (null: no folded bias)
    ws, nbytes = workspace(N, C, inp.get('sums'))
    args = (p(x), int(s['x_bf16']), p(cb), B, C, H, W, p(gamma), p(beta), p(mean), p(invstd), int(s['cl']),
            int(s['training']), s['lo'], s['hi'], p(dy), int(s['o_bf16']), int(s['tm']), p(dx), p(dgamma),
            p(dbeta), p(dcb), p(ws), nbytes)
    if op == 'bwd':
        N.check(L.asr_bn_act_bwd_f32(*args, st), 'asr_bn_act_bwd_f32')
    else:
        N.check(L.asr_bn_act_bwd_phase_f32(*args, int(op[-1]), float(inp.get('n_total', 0.0)), st),
                'asr_bn_act_bwd_phase_f32')
    torch.cuda.synchronize()
    return dict(dx=br.from_storage(host(dx), shape, xl), dgamma=host(dgamma), dbeta=host(dbeta),
                dconv_bias=host(dcb), sums=host(ws[:2 * C]))


def launch_wrapper(op, inp):
    """_native.bn_act_fwd / bn_act_bwd on channels-last storage of a C the channels-last kernels do
    not take: the wrapper goes down the NCHW path"""
    N = native()
    s = inp['spec']
    x = dev(inp['x']).contiguous(memory_format=torch.channels_last)
    gamma, beta, cb = dev(inp['gamma']), dev(inp['beta']), dev(inp['conv_bias'])
    if op == 'fwd':
        rm, rv = dev(inp['running_mean']), dev(inp['running_var'])
        out, mean, invstd = N.bn_act_fwd(x, gamma, beta, rm, rv, s['training'], inp['momentum'], inp['eps'],
                                         s['lo'], s['hi'], out_bf16=s['o_bf16'], time_major=s['tm'], conv_bias=cb)
        torch.cuda.synchronize()
        assert out.is_contiguous() and tuple(out.shape) == tuple(x.shape)
        return dict(out=host(out), save_mean=host(mean), save_invstd=host(invstd), running_mean=host(rm),
                    running_var=host(rv))
    dy = dev(inp['dy']).contiguous(memory_format=torch.channels_last)
    dx, dgamma, dbeta, dcb = N.bn_act_bwd(x, gamma, beta, dev(inp['save_mean']), dev(inp['save_invstd']),
                                          s['training'], s['lo'], s['hi'], dy, time_major=s['tm'], conv_bias=cb)
    torch.cuda.synchronize()
    return dict(dx=host(dx), dgamma=host(dgamma), dbeta=host(dbeta), dconv_bias=host(dcb), sums=None)


@pytest.mark.parametrize('name', CASES)
def test_launch_against_referee(name):
    op, inp, want, tol = prepared(name)
    got = (launch_wrapper if inp['spec']['via'] == 'wrapper' else launch_abi)(op, inp)
    stats = {}
    bad = br.judge(op, inp, got, want, tol, stats)
    for k in sorted(k for k in stats if not k.endswith(':share')):
        print('MEASURED %s %s error %.4g share of the bound %.3f' % (name, k, stats[k], stats[k + ':share']))
    assert not bad, bad
    if tol is None:                                     # the exact cases: equality, output by output
        for k, v in want.items():
            if k in got and got[k] is not None and v is not None and k != 'sums':
                assert torch.equal(torch.from_numpy(np.ascontiguousarray(got[k], dtype=np.float32)),
                                   torch.from_numpy(v.astype(np.float32))), k


# ---------------------------------------------------------------- gates: a refusal launches nothing

def _buffers(B, C, H, W, x_bf16=False):
    n = B * C * H * W
    t = dict(x=torch.zeros(n, dtype=torch.bfloat16 if x_bf16 else torch.float32, device=DEV),
             dy=torch.ones(n, device=DEV), vec=torch.ones(C, device=DEV),
             rm=torch.zeros(C, device=DEV), rv=torch.ones(C, device=DEV))
    for k in ('out', 'dx'):
        t[k] = poison(n, t['x'].dtype if k == 'dx' else torch.float32)
    for k in ('mean', 'invstd', 'dgamma', 'dbeta', 'dcb'):
        t[k] = poison(C)
    return t


def _fwd(N, t, B, C, H, W, cl, x_bf16=False, ws_bytes=None, null=()):
    ws, nbytes = workspace(N, C)
    a = {k: (None if k in null else N._p(v)) for k, v in t.items()}
    code = N.lib().asr_bn_act_fwd_f32(
        a['x'], int(x_bf16), None, B, C, H, W, a['vec'], a['vec'], a['rm'], a['rv'], int(cl), 1, 0.1, 1e-5, 0.0,
        20.0, a['out'], 0, 0, a['mean'], a['invstd'], None, None if 'ws' in null else N._p(ws),
        nbytes if ws_bytes is None else ws_bytes, N._stream())
    torch.cuda.synchronize()
    return code, ws


def _bwd(N, t, B, C, H, W, cl, x_bf16=False, ws_bytes=None, null=(), phase=0, n_total=0.0):
    ws, nbytes = workspace(N, C)
    a = {k: (None if k in null else N._p(v)) for k, v in t.items()}
    code = N.lib().asr_bn_act_bwd_phase_f32(
        a['x'], int(x_bf16), a['vec'], B, C, H, W, a['vec'], a['vec'], a['rm'], a['rv'], int(cl), 1, 0.0, 20.0,
        a['dy'], 0, 0, a['dx'], a['dgamma'], a['dbeta'], a['dcb'], None if 'ws' in null else N._p(ws),
        nbytes if ws_bytes is None else ws_bytes, phase, n_total, N._stream())
    torch.cuda.synchronize()
    return code, ws


def _all_poison(t, ws):
    return all(bool((t[k].float() == float(br.POISON)).all())
               for k in ('out', 'dx', 'mean', 'invstd', 'dgamma', 'dbeta', 'dcb')) and \
        bool((ws == float(br.POISON)).all())


def test_gates_refuse_and_leave_the_poison():
    N = native()
    refusals = []
    for C in (12, 2048):                                  # channels-last: C % 4, C / 4 | 256, C <= 1024
        t = _buffers(2, C, 3, 5)
        refusals += [(_fwd(N, t, 2, C, 3, 5, 1), N.ASR_EUNSUPPORTED, t), (_bwd(N, t, 2, C, 3, 5, 1), N.ASR_EUNSUPPORTED, t)]
    t = _buffers(2, 8, 3, 5, x_bf16=True)                 # bf16 x is a channels-last path
    refusals += [(_fwd(N, t, 2, 8, 3, 5, 0, x_bf16=True), N.ASR_EUNSUPPORTED, t),
                 (_bwd(N, t, 2, 8, 3, 5, 0, x_bf16=True), N.ASR_EUNSUPPORTED, t)]
    t = _buffers(2, 8, 3, 5)
    small = N.lib().asr_bn_act_workspace_bytes(8) - 1
    refusals += [(_fwd(N, t, 2, 8, 3, 5, 1, ws_bytes=small), N.ASR_EINVAL, t),
                 (_bwd(N, t, 2, 8, 3, 5, 1, ws_bytes=small), N.ASR_EINVAL, t),
                 (_fwd(N, t, 2, 8, 3, 5, 1, null=('ws',)), N.ASR_EINVAL, t),
                 (_bwd(N, t, 2, 8, 3, 5, 1, null=('ws',)), N.ASR_EINVAL, t)]
    for k in ('x', 'vec', 'out', 'mean', 'invstd'):
        refusals.append((_fwd(N, t, 2, 8, 3, 5, 1, null=(k,)), N.ASR_EINVAL, t))
    for k in ('x', 'vec', 'rm', 'rv', 'dy', 'dx', 'dgamma', 'dbeta'):      # (rm, rv: save_mean, save_invstd)
        refusals.append((_bwd(N, t, 2, 8, 3, 5, 1, null=(k,)), N.ASR_EINVAL, t))
    for n_total in (0.0, 0.5, -3.0, float('nan')):
        refusals.append((_bwd(N, t, 2, 8, 3, 5, 1, phase=2, n_total=n_total), N.ASR_EINVAL, t))
    refusals.append((_bwd(N, t, 2, 8, 3, 5, 1, phase=3), N.ASR_EINVAL, t))
    for (code, ws), want, t in refusals:
        assert code == want
        assert _all_poison(t, ws)
    # and the same buffers are taken once nothing is wrong; a null dconv_bias is accepted
    assert _fwd(N, t, 2, 8, 3, 5, 1)[0] == N.ASR_OK
    assert _bwd(N, t, 2, 8, 3, 5, 1, null=('dcb',))[0] == N.ASR_OK
    assert not (t['out'] == float(br.POISON)).any() and not (t['dx'] == float(br.POISON)).any()
    assert (t['dcb'] == float(br.POISON)).all()


def test_wrapper_takes_the_nchw_path_where_the_channels_last_kernels_refuse():
    names = [n for n in CASES if br.SPECS[n]['via'] == 'wrapper']
    assert sorted(br.SPECS[n]['C'] for n in names) == [6, 6, 12, 12]
    N = native()
    for C in (6, 12):
        t = _buffers(2, C, 4, 5)
        assert _fwd(N, t, 2, C, 4, 5, 1)[0] == N.ASR_EUNSUPPORTED      # the entry itself refuses
