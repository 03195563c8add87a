"""The referees of tests/rowwise_referee.py, proved on the CPU before they judge a kernel
(tests/test_rowwise_gpu.py):

* every reference is torch in double on the matrix's inputs (autograd for the backward ones) to
  1e-12 of the largest value; the bf16 halves are torch's bfloat16 conversion, bit for bit;
* the numpy fp32 model of the kernels' arithmetic passes every judge at every case: the bounds,
  measured per case against the reference alone, can be met by a correct implementation.
  Measured worst ratio of the model's error to the fp32 distance (torch.sum for the sums), where
  the error is above the 4 ulps every output is granted anyway: log-softmax y 1.5, its dx 5.0
  (lsm_bwd/edge_C2561), shifted dx 4.3 (edge_C2560), column sums 3.9.  The dx ratios above 4 are
  what rowwise_referee.wave_sum_term is derived for; with it the model uses at most 0.14 of the
  bound of a dx, 0.56 of that of nls and 0.83 of that of a column sum (stride_8197x5_ld8);
* the same model with one wrong term is rejected at the cases named in CAUGHT_AT.  Measured
  over the whole matrix (412 cases), cases that reject each mutant:

    dy_sum_drops_last_lane  104   every backward case with 64 columns or more
    exp_without_nls          97   every shifted backward case but the peaked rows (nls == 0)
    nls_wrong_sign           59
    mask_t_le_len           120
    lens_not_clamped         22   the cases with a length above T, and no other
    second_pass_dropped       7   the seven stride cases, and no other
    second_pass_reuses_rows   7   the same
    colsum_first_pass_only    1   shift_bwd_split/stride_8197x5_ld8
    padding_unset            55   every split case with ld > C
    bf16_truncates           87
    lo_from_x                90
    argmax_last_tie          12   the tie, all -inf, NaN and coarse cases, and no other
    argmax_ignores_lanes     24
    scale_touches_unit_rows  12   all of scale_rows: the signalling NaN of a factor-1 utterance
    sum_leading_skips_last   12   all of sum_leading with G > 1
"""
import numpy as np
import pytest
import torch

import rowwise_referee as rr

CASES = rr.cases()
IDS = ['%s/%s' % c for c in CASES]
_cache = {}


def prepared(op, name):
    """inputs, reference and tolerances of a case, made once"""
    key = (op, name)
    if key not in _cache:
        inp = rr.build(op, name)
        want = rr.reference(op, inp)
        _cache[key] = (inp, want) + rr.tolerances(op, inp, want)
    return _cache[key]


def test_the_matrix_is_what_it_claims():
    assert len(set(CASES)) == len(CASES)
    for op in rr.OPS:
        assert any(o == op for o, _ in CASES)
    for op, name in CASES:
        inp = rr.build(op, name)
        assert max(np.asarray(v).size for v in inp.values()) <= 1 << 20, (op, name)
    # a second pass of the grid-stride loops, and the block counts of the two-stage column sum
    assert rr.STRIDE_ROWS > rr.row_waves(rr.STRIDE_ROWS) == 32768
    assert rr.SPLIT_STRIDE_ROWS > 4 * rr.split_blocks(rr.SPLIT_STRIDE_ROWS) == 8192
    for nb in (31, 32, 33, 64, 2048):
        assert rr.split_blocks(rr.build('shift_bwd_split', 'blocks%d' % nb)['y'].shape[0]) == nb
    x = rr.build('lsm_fwd', 'stride_32771x3')['x']
    assert not np.array_equal(x[:3], x[32768:])                 # the second pass has rows of its own
    x = rr.build('lsm_fwd', 'peaked_C2401')['x']                # peaked: the fp32 sum is exactly 1
    assert (rr.model('shift_fwd', dict(x=x[:, None], lens=np.zeros(1, np.int32)))['nls'] == 0).all()
    x = rr.build('lsm_fwd', 'masked_C7')['x']
    assert np.isinf(x).any() and np.isfinite(x).any(-1).all()
    dy = rr.build('lsm_bwd', 'dy_zero_row_sums_C130')['dy']
    assert dy.any() and (rr._wave_sum(rr._lane_sum(rr._lanes(dy, 0.0))) == 0).all()


# ---------------------------------------------------------------- the references are torch in double

def _d(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _close12(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    scale = max(1.0, float(np.abs(want[fin]).max(initial=0.0)))
    assert float(np.abs(got[fin] - want[fin]).max(initial=0.0)) <= 1e-12 * scale


def _masked_sum(v, lens):
    T = v.shape[0]
    mask = torch.arange(T)[:, None] < torch.as_tensor(np.asarray(lens)).long().clamp(0, T)[None, :]
    return torch.where(mask, v, torch.zeros_like(v)).sum(0)


def _torch_bf16_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize('op,name', CASES, ids=IDS)
def test_reference_is_torch_in_double(op, name):
    inp, want = prepared(op, name)[:2]
    if op == 'lsm_fwd':
        _close12(want['y'], torch.log_softmax(_d(inp['x']), -1))
    elif op == 'lsm_bwd':                       # the case's y as logits: its log-softmax, unrounded
        x = _d(inp['y']).requires_grad_()
        lp = torch.log_softmax(x, -1)
        lp.backward(_d(inp['dy']))
        _close12(rr.ref_log_softmax_bwd(lp.detach().numpy(), inp['dy']), x.grad)
    elif op in ('sub_rowmax', 'shift_fwd'):
        x = _d(inp['x'])
        m = x.max(-1)[0]
        assert np.array_equal(want['y'], (x - m[..., None]).float().numpy(), equal_nan=True)
        if op == 'sub_rowmax':
            assert np.array_equal(want['row_max'], m.float().numpy())
            _close12(want['max_sum'], _masked_sum(m, inp['lens']))
        else:
            nls = torch.log_softmax(x, -1).max(-1)[0]
            _close12(want['nls'], nls)
            _close12(want['nls_sum'], _masked_sum(nls, inp['lens']))
    elif op in ('shift_bwd', 'shift_bwd_split'):
        x = _d(inp['y']).requires_grad_()
        lp = torch.log_softmax(x, -1)
        mx = lp.max(-1, keepdim=True)[0].detach()               # the reference detaches the maximum
        out = lp - mx
        out.backward(_d(inp['dy']))
        _close12(rr.ref_log_softmax_shift_bwd(out.detach().numpy(), mx[..., 0].numpy(), inp['dy']), x.grad)
        if op == 'shift_bwd_split':
            C = inp['y'].shape[-1]
            dx32 = want['dx'].astype(np.float32)
            hi = _torch_bf16_bits(dx32)
            assert np.array_equal(want['hi'][:, :C], hi)
            assert np.array_equal(want['lo'][:, :C], _torch_bf16_bits(dx32 - rr.bf16_f32(hi)))
            assert not want['hi'][:, C:].any() and not want['lo'][:, C:].any()
            _close12(want['colsum'], _d(want['dx']).sum(0))
    elif op == 'argmax':
        x = _d(inp['x'])
        idx = torch.max(torch.where(torch.isnan(x), torch.full_like(x, -rr.INF), x), -1)[1]
        assert np.array_equal(want['idx'], idx.numpy())
    elif op == 'sum_leading':
        t = _d(inp['t'])
        err = np.abs(want['out'] - t.sum(0).numpy())
        assert (err <= len(t) * 2.0 ** -24 * t.abs().sum(0).numpy()).all()
        if len(t) <= 2:
            assert np.array_equal(want['out'], t.sum(0).float().numpy())
    elif op == 'split_bf16':
        x = np.asarray(inp['x'], np.float32)
        ok = ~np.isnan(x)
        hi = _torch_bf16_bits(x)
        assert np.array_equal(want['hi'][ok], hi[ok])
        with np.errstate(invalid='ignore'):
            rest = x - rr.bf16_f32(hi)
        ok &= ~np.isnan(rest)
        assert np.array_equal(want['lo'][ok], _torch_bf16_bits(rest)[ok])
        assert np.isnan(rr.bf16_f32(want['hi'][np.isnan(x)])).all() and np.isnan(rr.bf16_f32(want['lo'][np.isnan(rest)])).all()
        # the exact pair where it is finite: hi + lo is x to 2^-16 (2^-17 but for lo's own rounding)
        fin = np.isfinite(rr.bf16_f32(want['hi'])) & np.isfinite(x)
        with np.errstate(invalid='ignore'):
            s = rr.bf16_f32(want['hi']).astype(np.float64) + rr.bf16_f32(want['lo']).astype(np.float64)
        assert (np.abs(s[fin] - x[fin]) <= 2.0 ** -16 * np.abs(x)[fin] + 2.0 ** -133).all()
    elif op == 'scale_rows':
        x, sc = torch.from_numpy(inp['x']), torch.from_numpy(inp['scale'])
        keep = inp['scale'] == 1
        assert np.array_equal(rr.f32_bits(want['x'][:, keep]), rr.f32_bits(inp['x'][:, keep]))
        assert np.array_equal(rr.f32_bits(want['x'][:, ~keep]), rr.f32_bits((x * sc[None, :, None]).numpy()[:, ~keep]))
    else:
        raise KeyError(op)


def test_special_values_of_the_contract():
    """what include/asr_amd.h says about -inf rows, NaN and +-inf, as the references have it"""
    y = rr.ref_log_softmax_fwd(np.array([[-rr.INF] * 3, [0.0, -rr.INF, 0.0]], np.float32))
    assert np.isnan(y[0]).all() and y[1, 1] == -rr.INF and np.isfinite(y[1, [0, 2]]).all()
    f = rr.ref_log_softmax_shift_fwd(np.full((1, 1, 4), -rr.INF, np.float32), [1])
    assert np.isnan(f['y']).all() and np.isnan(f['nls']).all()
    assert rr.ref_argmax_rows(np.array([[rr.NAN, 1.0, 2.0, 2.0], [rr.NAN, -rr.INF, rr.NAN, -rr.INF]], np.float32)).tolist() == [2, 0]
    hi, lo = rr.ref_split_bf16(np.array([0x7f800000, 0xff800000, 0x7fc00000, 0x7f7f8000], np.uint32).view(np.float32))
    assert hi[:2].tolist() == [0x7f80, 0xff80] and np.isnan(rr.bf16_f32(lo[:2])).all()
    assert np.isnan(rr.bf16_f32(hi[2])) and np.isnan(rr.bf16_f32(lo[2]))
    assert (hi[3], lo[3]) == (0x7f80, 0xff80)                   # rounds to inf: lo = x - inf
    # a rest just short of half a step rounds up to it: odd hi on an exact tie of hi + lo is a
    # correct split, which is why the split judge takes either neighbour there
    hi, lo = rr.ref_split_bf16(np.array([0x3f817fff], np.uint32).view(np.float32))
    assert (hi[0], lo[0]) == (0x3f81, 0x3b80)


# ---------------------------------------------------------------- the bounds can be met

@pytest.mark.parametrize('op,name', CASES, ids=IDS)
def test_fp32_model_passes_every_judge(op, name):
    inp, want, tol, dist = prepared(op, name)
    stats = {}
    bad = rr.judge(op, inp, rr.model(op, inp), want, tol, stats)
    print(op, name, {k: '%.3g (fp32 distance %.3g)' % (stats[k], dist[k]) for k in rr.FLOATING.get(op, ())})
    assert not bad, bad


def test_the_yardstick_is_no_kernel():
    """the tolerance comes from the inputs and the reference alone"""
    inp, want, tol, dist = prepared('shift_bwd', 'edge_C129')
    tol2, dist2 = rr.tolerances('shift_bwd', {k: np.array(v, copy=True) for k, v in inp.items()}, want)
    assert dist == dist2 and all(np.array_equal(tol[k], tol2[k]) for k in tol)
    assert dist['dx'] > 0 and float(np.max(tol['dx'])) < 1e-4


# ---------------------------------------------------------------- the mutants are rejected

S = 'stride_%dx%d' % (rr.STRIDE_ROWS, rr.STRIDE_C)
SS = 'stride_%dx%d_ld%d' % (rr.SPLIT_STRIDE_ROWS, rr.SPLIT_STRIDE_C, rr.SPLIT_STRIDE_LD)
STRIDES = [(op, S) for op in rr.ROW_OPS] + [('shift_bwd_split', SS)]
# mutant -> cases of the matrix that must reject it
CAUGHT_AT = {
    'dy_sum_drops_last_lane': [('lsm_bwd', 'edge_C64'), ('shift_bwd', 'edge_C129'), ('shift_bwd_split', 'edge_C64_ld64')],
    'exp_without_nls': [('shift_bwd', 'edge_C65'), ('shift_bwd_split', 'edge_C65_ld72')],
    'nls_wrong_sign': [('shift_fwd', 'edge_C2'), ('shift_fwd', 'randn30_C130')],
    'mask_t_le_len': [('sub_rowmax', 'lens_T64_B5'), ('shift_fwd', 'lens_T65_B1_len0')],
    'lens_not_clamped': [('sub_rowmax', 'lens_T1_B1_len4'), ('shift_fwd', 'lens_T130_B5')],
    'second_pass_dropped': STRIDES,
    'second_pass_reuses_rows': STRIDES,
    'colsum_first_pass_only': [('shift_bwd_split', SS)],
    'padding_unset': [('shift_bwd_split', 'next_class_C120_ld192'), ('shift_bwd_split', 'edge_C1_ld8')],
    'bf16_truncates': [('split_bf16', 'specials'), ('split_bf16', 'dense_3x7'), ('shift_bwd_split', 'edge_C64_ld64')],
    'lo_from_x': [('split_bf16', 'specials'), ('split_bf16', 'strided_x_9x5'), ('shift_bwd_split', 'edge_C64_ld64')],
    'argmax_last_tie': [('argmax', 'tie_c_c64'), ('argmax', 'tie_c_c1'), ('argmax', 'tie_all_lanes_64')],
    'argmax_ignores_lanes': [('argmax', 'edge_C65'), ('argmax', 'edge_C64'), ('argmax', 'tie_c_c1')],
    'scale_touches_unit_rows': [('scale_rows', 'T1_C1'), ('scale_rows', 'T9_C257')],
    'sum_leading_skips_last': [('sum_leading', 'G2_n4'), ('sum_leading', 'G64_n1028')],
}
# ... and cases that cannot tell it from the real thing, as it must be
BLIND_AT = {
    'exp_without_nls': [('shift_bwd', 'peaked_C130')],                  # nls == 0
    'dy_sum_drops_last_lane': [('lsm_bwd', 'edge_C63'), ('lsm_bwd', 'dy_zero_C130')],
    'lens_not_clamped': [('sub_rowmax', 'lens_T64_B1_len-2')],          # a negative length sums nothing
    'second_pass_dropped': [('lsm_fwd', 'edge_C1024')],
    'argmax_last_tie': [('argmax', 'edge_C129')],
    'padding_unset': [('shift_bwd_split', 'edge_C64_ld64')],
    'sum_leading_skips_last': [('sum_leading', 'G1_n1024')],
}


def test_every_mutant_has_its_cases():
    assert set(CAUGHT_AT) == set(rr.MUTANTS)
    assert all(c in CASES for cs in list(CAUGHT_AT.values()) + list(BLIND_AT.values()) for c in cs)


@pytest.mark.parametrize('mut', rr.MUTANTS)
def test_mutant_is_rejected(mut):
    for op, name in CAUGHT_AT[mut]:
        inp, want, tol, _ = prepared(op, name)
        bad = rr.judge(op, inp, rr.model(op, inp, mut), want, tol)
        print(mut, op, name, bad[:2])
        assert bad, (mut, op, name)
    for op, name in BLIND_AT.get(mut, ()):
        inp, want, tol, _ = prepared(op, name)
        assert not rr.judge(op, inp, rr.model(op, inp, mut), want, tol), (mut, op, name)


def test_split_judge_wants_nearest_halves():
    """the judge of the split backward takes any fp32 d within tolerance, and nothing that is not
    split(d): hi one bf16 step off with lo making up for it is no RNE split"""
    inp, want, tol, _ = prepared('shift_bwd_split', 'edge_C65_ld72')
    got = rr.model('shift_bwd_split', inp)
    assert not rr.judge('shift_bwd_split', inp, got, want, tol)
    hi = got['hi'].copy()
    hi[3, 5] += 1
    d = rr.bf16_f32(got['hi'][3, 5:6]).astype(np.float64) + rr.bf16_f32(got['lo'][3, 5:6]).astype(np.float64)
    lo = got['lo'].copy()
    lo[3, 5] = rr.bf16_rne((d - rr.bf16_f32(hi[3, 5:6])).astype(np.float32))[0]
    bad = rr.judge('shift_bwd_split', inp, dict(got, hi=hi, lo=lo), want, tol)
    assert any('nearest' in b for b in bad), bad
    lo = got['lo'].copy()
    lo[3, 70] = 0x8000                                          # -0 in a padded column
    assert rr.judge('shift_bwd_split', inp, dict(got, lo=lo), want, tol)
