"""The referee of tests/bn_referee.py, proved on the CPU before it judges a kernel
(tests/test_bn_referee_gpu.py):

* every reference is torch.float64 nn.BatchNorm2d + nn.Hardtanh (autograd for the backward ones)
  on the matrix's inputs to 1e-12 of the largest value, the running statistics and the
  num_batches_tracked / momentum choice of native_bn.batch_stats_config included, NaN for NaN;
* the numpy fp32 model of the kernels' arithmetic passes every judge at every case: the derived
  bounds can be met (largest share of a bound the model uses: save_mean 0.49 and save_invstd 0.38
  where chan_sums leave one fp32 rounding, running statistics 0.13, gradient sums 0.04; a bf16
  output may fill its interval: the bounds are worst-case linear in the depth); in the exact-integer cases it equals the
  reference;
* the same model with one wrong term is rejected at the case named in CAUGHT_AT;
* with the reference's own values no case leaves more than 1 element in 1000 out near a clamp;
* the matrix reaches every kernel instantiation the launchers can select."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import bn_referee as br

CASES = br.cases()
_cache = {}

CAUGHT_AT = {
    'mask_le_hi': 'bwd/exact_nchw_B3C3H9W37',
    'mask_ge_lo': 'bwd/exact_lohi_nhwc4_B3C64H5W11',
    'slice_last_pixel_dropped': 'fwd/nhwc4_B3C32H5W11',
    'second_trip_dropped': 'bwd/nhwc8_obf16_B4C128H9W57',
    'tile_row_from_wrong_batch': 'bwd/tm_xf32_of32_B5C32H3W11',
    'channels_ge_256_missing': 'fwd/nhwc4_B3C512H5W11',
    'biased_running_var': 'fwd/nhwc4_B3C32H5W11',
    'bias_missing_from_mean': 'fwd/nhwc4_bias_B3C64H5W11',
    'k2_dropped': 'bwd/nchw_of32_tm0_B2C3H5W7',
    'bf16_truncates': 'fwd/nchw_obf16_tm0_B2C3H5W7',
    'nan_clamped_to_lo': 'fwd/nan_eval_nchw_B2C3H5W7',
    'tm_index_b_h_swapped': 'fwd/tm_xf32_of32_B5C32H3W11',
}


def prepared(name):
    """inputs, reference and tolerances (None: an exact case) of a case, made once"""
    if name not in _cache:
        inp = br.build(name)
        op = inp['spec']['op']
        want = br.reference(op, inp)
        tol = None if inp['spec']['kind'] == 'exact' else br.tolerances(op, inp, want)
        _cache[name] = (op, inp, want, tol)
    return _cache[name]


def test_the_matrix_is_what_it_claims():
    assert len(set(CASES)) == len(CASES)
    reached = set()
    for name in CASES:
        s = br.SPECS[name]
        assert s['B'] * s['C'] * s['H'] * s['W'] <= 2 << 20, name
        reached |= set(br.families(s))
    assert reached == br.ALL_FAMILIES, (br.ALL_FAMILIES - reached, reached - br.ALL_FAMILIES)
    assert set(CAUGHT_AT) == set(br.MUTANTS) and set(CAUGHT_AT.values()) <= set(CASES)
    for op in br.OPS:
        assert any(br.SPECS[n]['op'] == op for n in CASES)
    # the caps of the two launch geometries, the tile rows, the grid-stride trips
    s = br.SPECS['fwd/nhwc4_cap_B1C4H1W262181']
    assert br.nwg(s['W']) == 4096 and -(-s['W'] // 4096) == 65
    s = br.SPECS['fwd/tm_cap_w1_B2341C8H7W1']
    assert -(-s['B'] * s['H'] // br.tm_rows(8)) == 2049
    assert [br.tm_rows(cw) for cw in (352, 2048, 12288)] == [8, 6, 1] and br.tm_rows(13312) == 0
    for C, trips in ((128, 3), (256, 5)):
        P = 4 * 9 * 57
        assert -(-P // (2 * (2048 // C) * br.nwg(P))) == trips
    paths = {br.apply_path(br.SPECS[n]) for n in CASES}
    assert paths == {'nchw', 'nhwc4', 'nhwc8', 'tm'}
    assert br.apply_path(br.SPECS['fwd/nhwc4_tm_wide_B2C1024H3W13']) == 'nhwc4'
    assert br.apply_path(br.SPECS['fwd/nhwc4_xbf16_obf16_tm1_B3C4H7W5']) == 'nhwc4'
    # a tile of 8 rows at H = 3 spans three utterances
    assert {r // 3 for r in range(8)} == {0, 1, 2}


# ---------------------------------------------------------------- the references are torch in double

def _close12(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = ~np.isnan(want)
    scale = max(1.0, float(np.abs(want[fin]).max(initial=0.0)))
    assert float(np.abs(got[fin] - want[fin]).max(initial=0.0)) <= 1e-12 * scale, what


def _torch_module(inp):
    spec = inp['spec']
    null = inp['running_mean'] is None
    # (torch refuses the exact cases' eps = 0; 1e-300 vanishes in running_var + eps)
    bn = nn.BatchNorm2d(spec['C'], eps=float(np.float32(inp['eps'])) or 1e-300, momentum=float(np.float32(inp['momentum'])),
                        track_running_stats=not null).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(inp['gamma'].astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(inp['beta'].astype(np.float64)))
        if not null:
            bn.running_mean.copy_(torch.from_numpy(inp['running_mean'].astype(np.float64)))
            bn.running_var.copy_(torch.from_numpy(inp['running_var'].astype(np.float64)))
    bn.train(spec['training'])
    return bn


def _torch_run(inp, dy=None):
    spec = inp['spec']
    bn = _torch_module(inp)
    x = torch.from_numpy(inp['x'].astype(np.float64)).requires_grad_()
    cb = None
    v = x
    if inp['conv_bias'] is not None:
        cb = torch.from_numpy(inp['conv_bias'].astype(np.float64)).requires_grad_()
        v = x + cb[None, :, None, None]
    y = nn.Hardtanh(spec['lo'], spec['hi'])(bn(v))
    if dy is not None:
        y.backward(torch.from_numpy(dy.astype(np.float64)))
    return bn, x, cb, y.detach().numpy()


NON_PHASE = [n for n in CASES if br.SPECS[n]['op'] in ('fwd', 'bwd')]


@pytest.mark.parametrize('name', NON_PHASE)
def test_reference_is_torch_in_double(name):
    from att_speech.modules.encoders.native_bn import batch_stats_config
    op, inp, want, _ = prepared(name)
    spec = inp['spec']
    if inp['n'] == 1 and spec['training']:      # torch refuses one value per channel: by hand
        if op == 'fwd':
            be = inp['beta'].astype(np.float64)
            assert np.array_equal(want['out'].reshape(-1), np.clip(be, spec['lo'], spec['hi']))
            assert np.array_equal(want['save_mean'], inp['x'].reshape(-1).astype(np.float64))
            mom = float(np.float32(inp['momentum']))
            _close12(want['running_var'], (1 - mom) * inp['running_var'].astype(np.float64), name)
        else:
            assert not want['dx'].any()          # xhat = 0, dy' - mean(dy') = 0
        return
    if op == 'fwd':
        fwd = dict(inp)
        if spec['chan_sums']:
            # the sums the case hands over are those of its x: the reference from x must agree
            direct = br.reference('fwd', dict(inp, spec=dict(spec, chan_sums=False)))
            for k in ('out', 'save_mean', 'save_invstd', 'running_mean', 'running_var'):
                _close12(want[k], direct[k], k)
        bn, _, _, y = _torch_run(fwd)
        _close12(want['out'], y, 'out')
        # the module as the wrapper sees it: which statistics, which momentum, the step counter
        probe = _torch_module(inp)
        use_batch, momentum, rm, rv = batch_stats_config(probe)
        assert use_batch == spec['training']
        if inp['running_mean'] is None:
            assert rm is None and rv is None and bn.running_mean is None
            assert want['running_mean'] is None and want['running_var'] is None
        else:
            assert rm is probe.running_mean and rv is probe.running_var
            assert int(probe.num_batches_tracked) == int(bn.num_batches_tracked) == int(spec['training'])
            if spec['training']:
                assert momentum == float(np.float32(inp['momentum']))
            _close12(want['running_mean'], bn.running_mean.numpy(), 'running_mean')
            _close12(want['running_var'], bn.running_var.numpy(), 'running_var')
        if spec['training']:
            v = inp['x'].astype(np.float64) + br._c(br._bias(inp))
            vt = torch.from_numpy(v)
            _close12(want['save_mean'], vt.mean((0, 2, 3)), 'save_mean')
            _close12(want['save_invstd'], (vt.var((0, 2, 3), unbiased=False) + bn.eps).rsqrt(), 'save_invstd')
        return
    # backward: torch differentiates through its own fp64 statistics; the reference is given them unrounded
    st = br._ref_stats(dict(inp, spec=dict(spec, chan_sums=False)))
    got = br._ref_bwd(inp, mean=st['mean'], invstd=st['invstd'])
    bn, x, cb, _ = _torch_run(inp, inp['dy'])
    _close12(got['dx'], x.grad.numpy(), 'dx')
    _close12(got['dgamma'], bn.weight.grad.numpy(), 'dgamma')
    _close12(got['dbeta'], bn.bias.grad.numpy(), 'dbeta')
    if cb is not None:
        # in training mode torch's bias gradient is rounding noise around the reference's exact 0
        tgt = cb.grad.numpy()
        if spec['training']:
            assert not got['dconv_bias'].any()
            assert float(np.abs(tgt).max()) <= 1e-9 * max(1.0, float(np.abs(got['dbeta']).max()))
        else:
            _close12(got['dconv_bias'], tgt, 'dconv_bias')


@pytest.mark.parametrize('name', [n for n in CASES if br.SPECS[n]['op'].startswith('bwd_phase')])
def test_phase_references_are_the_two_halves_of_the_whole(name):
    """phase 1 leaves the sums and parameter gradients of the whole backward; phase 2 on the doubled
    sums of two replicas with the same data and n_total = 2 n gives the whole backward's dx"""
    op, inp, want, _ = prepared(name)
    whole = br._ref_bwd(dict(inp, spec=dict(inp['spec'], op='bwd')))
    if op == 'bwd_phase1':
        assert want['dx'] is None
        assert np.array_equal(want['sums'][0::2], whole['dbeta']) and np.array_equal(want['sums'][1::2], whole['dgamma'])
        assert np.array_equal(want['dgamma'], whole['dgamma'])
    else:
        assert inp['n_total'] == 2 * inp['n'] and want['dgamma'] is None and want['dbeta'] is None
        _close12(want['dx'], whole['dx'], 'dx')


# ---------------------------------------------------------------- the bounds can be met; the cap holds

@pytest.mark.parametrize('name', CASES)
def test_model_passes_the_judge(name):
    op, inp, want, tol = prepared(name)
    stats = {}
    bad = br.judge(op, inp, br.model(op, inp), want, tol, stats)
    assert not bad, bad
    if tol is not None and op != 'fwd':
        assert tol['ambiguous'].sum() <= br.left_out_cap(inp['spec'])


@pytest.mark.parametrize('name', br.exact_cases())
def test_exact_cases_are_exact(name):
    op, inp, want, tol = prepared(name)
    assert tol is None
    spec = inp['spec']
    for k, v in want.items():
        if k in ('out', 'save_mean', 'save_invstd', 'dx', 'dgamma', 'dbeta', 'dconv_bias') and v is not None:
            assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), k     # an fp32 number
            if spec['o_bf16' if k == 'out' else 'x_bf16'] and k in ('out', 'dx'):
                assert np.array_equal(v, br._bf(v).astype(np.float64)), k             # a bf16 number
    y = want['y']
    share = y.size // 200
    assert (y == spec['lo']).sum() >= share and (y == spec['hi']).sum() >= share      # many ON each clamp
    assert (y < spec['lo']).any() and (y > spec['hi']).any() and ((y > spec['lo']) & (y < spec['hi'])).any()
    got = br.model(op, inp)
    for k in (('out', 'save_mean', 'save_invstd') if op == 'fwd' else ('dx', 'dgamma', 'dbeta', 'dconv_bias')):
        assert np.array_equal(np.asarray(got[k], np.float64), want[k]), k


# ---------------------------------------------------------------- every mutant is rejected

@pytest.mark.parametrize('mut', br.MUTANTS)
def test_mutant_is_rejected(mut):
    op, inp, want, tol = prepared(CAUGHT_AT[mut])
    assert not br.judge(op, inp, br.model(op, inp), want, tol)
    bad = br.judge(op, inp, br.model(op, inp, mut), want, tol)
    assert bad, mut
    print('MUTANT %-28s rejected at %s: %s' % (mut, CAUGHT_AT[mut], bad[0]))


def test_judge_sees_what_a_launch_must_leave_alone():
    op, inp, want, tol = prepared('bwd_phase1/nhwc4_bias_B3C64H5W11')
    got = br.model(op, inp)
    assert (got['dx'] == br.POISON).all()
    got['dx'][1, 2, 3, 4] = 0.0
    assert any(b.startswith('dx') for b in br.judge(op, inp, got, want, tol))
    op, inp, want, tol = prepared('bwd_phase2/nhwc4_bias_B3C64H5W11')
    got = br.model(op, inp)
    assert not br.judge(op, inp, got, want, tol)
    for k in ('dgamma', 'dbeta', 'dconv_bias'):
        g2 = copy.deepcopy(got)
        g2[k][5] = 1.0
        assert any(b.startswith(k) for b in br.judge(op, inp, g2, want, tol))
    g2 = copy.deepcopy(got)
    g2['sums'] = got['sums'] * 0.5
    assert br.judge(op, inp, g2, want, tol)


def test_storage_orders_round_trip():
    a = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)
    for lay in ('nchw', 'nhwc', 'tm'):
        assert np.array_equal(br.from_storage(br.to_storage(a, lay), a.shape, lay), a)
    assert br.to_storage(a, 'tm')[((4 * 2 + 1) * 3 + 2) * 7 + 6] == a[1, 2, 4, 6]
    assert br.to_storage(a, 'nhwc')[((1 * 5 + 4) * 7 + 6) * 3 + 2] == a[1, 2, 4, 6]
