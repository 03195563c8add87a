"""The row-wise normaliser kernels of csrc/softmax.hip and asr_scale_rows_f32, one launch at a time
against the fp64 referees of tests/rowwise_referee.py (proved on the CPU by
tests/test_rowwise_referee.py, which also shows that this matrix rejects fifteen one-term
mutants): class edges on both sides of every PER instantiation, a second pass of every
grid-stride loop, the block counts of the two-stage column sum, peaked / masked / constant /
offset / wide-spread logits, five kinds of dy, lengths outside [0, T], ties and NaN for the
arg-max, the special values and the three kernels of the bf16 split.

Exact outputs are held bit for bit.  Floating outputs are held to 4x the distance of the plain
fp32 CPU evaluation from fp64 plus 4 fp32 ulps of the largest value of the row (for sums: of the
largest summand or the sum), per case.

Measured on the MI355X over the 412 cases, per entry point and floating output: the worst ratio
of the kernel's error to the fp32 CPU distance (and its case), and the largest share of its bound
that any entry uses.  No case exceeds its bound, so no term was derived for __expf / __logf:

    asr_log_softmax_fwd_f32        y        3.3  constant_C2401 (6.9e-7 / 2.1e-7, under an ulp of |y| = 7.8)   0.15
    asr_log_softmax_bwd_f32        dx       1.6  dy_one_hot_C7                                               0.18
    asr_sub_rowmax_f32             max_sum  7.0  randn30_C130 (5.3e-5 / 7.6e-6, half an ulp of the sum)      0.14
    asr_log_softmax_shift_fwd_f32  nls      3.3  constant_C2401                                              0.25
                                   nls_sum  4.8  randn4_C7 (2.0e-7 / 4.1e-8)                                 0.36
    asr_log_softmax_shift_bwd_f32  dx       1.5  dy_posterior_C7                                             0.18
    ..._shift_bwd_split_bf16       hi + lo  159  constant_C2401 (2.0e-5: the 2^-16 of lo, not fp32)          0.46
                                   colsum   2.1  edge_C2_ld2                                                 0.22

(ratios above 4 are errors inside the 4 ulps every output is granted.)  Everything exact is exact:
sub_rowmax y and row_max, the shifted y, argmax, the bf16 halves, sum_leading, scale_rows.

What this file found: asr_log_softmax_fwd_f32 computed x - (max + log s), which rounds log s to
an ulp of the maximum: at lsm_fwd/offset1e4_C7, _C130 and _C2401 (logits around 1e4) every value
was off by up to 4.6e-4, 60x the bound; it now computes (x - max) - log s.  asr_argmax_rows_f32
let a NaN freeze its lane of the butterfly, losing the maxima that lane had gathered
(argmax/nan_ranks_as_minus_inf: column 0 for a maximum in column 37); a NaN now ranks as -inf.
Both were measured on the MI355X with the kernels as they were: these four cases failed, the
other 408 passed.

The outputs of the matrix come from the wrappers' torch.empty, where a row that a launch skips
holds whatever was there before; the stride cases therefore run a second time through the C
entries on buffers filled with POISON (test_stride_passes_write_every_row)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import rowwise_referee as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = rr.cases()
IDS = ['%s/%s' % c for c in CASES]
_cache = {}


def native():
    from att_speech import _native
    return _native


def prepared(op, name):
    key = (op, name)
    if key not in _cache:
        inp = rr.build(op, name)
        want = rr.reference(op, inp)
        _cache[key] = (inp, want) + rr.tolerances(op, inp, want)
    return _cache[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def bits16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def poisoned_halves(rows, ld):
    return torch.full((rows, ld), rr.POISON_H, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def one_float_in(a):
    """a contiguous device copy of `a` that starts 4 bytes into its allocation"""
    base = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    view = base[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def launch_split_bf16(N, inp):
    x = np.asarray(inp['x'], np.float32)
    mode, gap = inp['mode'], inp.get('gap', 0)
    if x.ndim == 1:                             # one contiguous row: the wrapper allocates
        hi, lo = N.split_bf16(dev(x) if mode == 'contiguous' else one_float_in(x))
        return dict(hi=bits16(hi), lo=bits16(lo))
    rows, cols = x.shape
    bh, bl = poisoned_halves(rows, cols + gap), poisoned_halves(rows, cols + gap)
    if mode == 'strided_x':                     # the wrapper would copy a strided x: the entry itself
        ldx = cols + inp['xgap']
        xb = torch.full((rows, ldx), 7.0, device=DEV)
        xb[:, :cols] = dev(x)
        N.check(N.lib().asr_split_bf16_f32(N._p(xb), rows, cols, ldx, N._p(bh), cols + gap, N._p(bl), cols + gap,
                                           N._stream()), 'asr_split_bf16_f32')
    else:
        N.split_bf16(dev(x) if mode == 'dense' else one_float_in(x), bh[:, :cols], bl[:, :cols])
    return dict(hi=bits16(bh), lo=bits16(bl))


def launch(op, inp):
    """one launch through att_speech._native -> the outputs as rowwise_referee.judge takes them"""
    N = native()
    if op == 'lsm_fwd':
        out = dict(y=N.log_softmax_fwd(dev(inp['x']), inp['x'].shape[-1]))
    elif op == 'lsm_bwd':
        out = dict(dx=N.log_softmax_bwd(dev(inp['y']), dev(inp['dy']), inp['y'].shape[-1]))
    elif op == 'sub_rowmax':
        out = dict(zip(('y', 'row_max', 'max_sum'), N.sub_rowmax(dev(inp['x']), dev(inp['lens']))))
    elif op == 'shift_fwd':
        out = dict(zip(('y', 'nls', 'nls_sum'), N.log_softmax_shift_fwd(dev(inp['x']), dev(inp['lens']))))
    elif op == 'shift_bwd':
        out = dict(dx=N.log_softmax_shift_bwd(dev(inp['y']), dev(inp['nls']), dev(inp['dy'])))
    elif op == 'shift_bwd_split':
        hi, lo, cs = N.log_softmax_shift_bwd_split(dev(inp['y']), dev(inp['nls']), dev(inp['dy']), inp['ld'])
        torch.cuda.synchronize()
        return dict(hi=bits16(hi), lo=bits16(lo), colsum=host(cs))
    elif op == 'argmax':
        out = dict(idx=N.argmax_rows(dev(inp['x'])))
    elif op == 'sum_leading':
        t = dev(inp['t'])
        assert t.data_ptr() % 16 == 0           # the kernel, not the wrapper's torch.sum
        out = dict(out=N.sum_leading(t))
    elif op == 'scale_rows':
        out = dict(x=N.scale_rows_(dev(inp['x']), dev(inp['scale'])))
    elif op == 'split_bf16':
        out = launch_split_bf16(N, inp)
        torch.cuda.synchronize()
        return out
    else:
        raise KeyError(op)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize('op,name', CASES, ids=IDS)
def test_launch_against_referee(op, name):
    inp, want, tol, dist = prepared(op, name)
    got = launch(op, inp)
    stats = {}
    bad = rr.judge(op, inp, got, want, tol, stats)
    for k in rr.FLOATING.get(op, ()):
        print('MEASURED %s %s %s error %.4g fp32 distance %.4g share of the bound %.3f' % (
            op, name, k, stats[k], dist[k], stats[k + ':share']))
    assert not bad, bad


def launch_poisoned(op, inp):
    """the C entry itself on outputs pre-filled with POISON: a skipped row is certain to show"""
    N = native()
    L, st, p = N.lib(), N._stream(), N._p

    def full(shape, value=float(rr.POISON), dtype=torch.float32):
        return torch.full(tuple(shape), value, dtype=dtype, device=DEV)
    if op in ('lsm_fwd', 'argmax'):
        x = dev(inp['x'])
        if op == 'lsm_fwd':
            out = dict(y=full(x.shape))
            N.check(L.asr_log_softmax_fwd_f32(p(x), x.shape[0], x.shape[1], p(out['y']), st), op)
        else:
            out = dict(idx=full(x.shape[:1], rr.POISON_I, torch.int32))
            N.check(L.asr_argmax_rows_f32(p(x), x.shape[0], x.shape[1], p(out['idx']), st), op)
    elif op in ('sub_rowmax', 'shift_fwd'):
        x, lens = dev(inp['x']), dev(inp['lens'])
        T, B, C = x.shape
        names = ('y', 'row_max', 'max_sum') if op == 'sub_rowmax' else ('y', 'nls', 'nls_sum')
        out = dict(zip(names, (full(x.shape), full((T, B)), full((B,)))))
        fn = L.asr_sub_rowmax_f32 if op == 'sub_rowmax' else L.asr_log_softmax_shift_fwd_f32
        N.check(fn(p(x), T, B, C, p(lens), *[p(out[k]) for k in names], st), op)
    elif op in ('lsm_bwd', 'shift_bwd'):
        y, dy = dev(inp['y']), dev(inp['dy'])
        out = dict(dx=full(y.shape))
        if op == 'lsm_bwd':
            N.check(L.asr_log_softmax_bwd_f32(p(y), p(dy), y.shape[0], y.shape[1], p(out['dx']), st), op)
        else:
            N.check(L.asr_log_softmax_shift_bwd_f32(p(y), p(dev(inp['nls'])), p(dy), y.shape[0], y.shape[1],
                                                    p(out['dx']), st), op)
    elif op == 'shift_bwd_split':
        y, nls, dy, ld = dev(inp['y']), dev(inp['nls']), dev(inp['dy']), inp['ld']
        rows, C = y.shape
        hi, lo = poisoned_halves(rows, ld), poisoned_halves(rows, ld)
        part = full((L.asr_log_softmax_shift_bwd_split_blocks(rows), ld))
        N.check(L.asr_log_softmax_shift_bwd_split_bf16(p(y), p(nls), p(dy), rows, C, p(hi), p(lo), ld, p(part), st), op)
        torch.cuda.synchronize()
        return dict(hi=bits16(hi), lo=bits16(lo), colsum=host(part).astype(np.float64).sum(0)[:C])
    else:
        raise KeyError(op)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


STRIDE_CASES = [(op, 'stride_%dx%d' % (rr.STRIDE_ROWS, rr.STRIDE_C)) for op in rr.ROW_OPS] + [
    ('shift_bwd_split', 'stride_%dx%d_ld%d' % (rr.SPLIT_STRIDE_ROWS, rr.SPLIT_STRIDE_C, rr.SPLIT_STRIDE_LD))]


@pytest.mark.parametrize('op,name', STRIDE_CASES, ids=['%s/%s' % c for c in STRIDE_CASES])
def test_stride_passes_write_every_row(op, name):
    inp, want, tol, _ = prepared(op, name)
    assert (op, name) in CASES
    bad = rr.judge(op, inp, launch_poisoned(op, inp), want, tol)
    assert not bad, bad


FIXED_ORDER_CASES = [('sub_rowmax', 'stride_32771x3'), ('sub_rowmax', 'lens_T130_B5'),
                     ('shift_fwd', 'stride_32771x3'), ('shift_fwd', 'lens_T130_B5'),
                     ('shift_bwd_split', 'stride_8197x5_ld8'), ('shift_bwd_split', 'blocks64'),
                     ('shift_bwd_split', 'blocks33'), ('shift_bwd_split', 'edge_C2401_ld2408')]


@pytest.mark.parametrize('op,name', FIXED_ORDER_CASES, ids=['%s/%s' % c for c in FIXED_ORDER_CASES])
def test_fixed_order_sums_repeat_bit_for_bit(op, name):
    inp = prepared(op, name)[0]
    a, b = launch(op, inp), launch(op, inp)
    for k in rr.FIXED_ORDER[op]:
        assert np.array_equal(rr.f32_bits(a[k]), rr.f32_bits(b[k])), k


# ---------------------------------------------------------------- argument checks: nothing is launched

def test_unsupported_widths_and_bad_arguments():
    N = native()
    L = N.lib()
    C = rr.UNSUPPORTED_C
    x = torch.zeros(1, 1, C, device=DEV)
    lens = torch.ones(1, dtype=torch.int32, device=DEV)
    nls = torch.zeros(1, device=DEV)
    for call in (lambda: N.log_softmax_fwd(x, C), lambda: N.log_softmax_bwd(x, x, C),
                 lambda: N.sub_rowmax(x, lens), lambda: N.log_softmax_shift_fwd(x, lens),
                 lambda: N.log_softmax_shift_bwd(x[0], nls, x[0]), lambda: N.argmax_rows(x)):
        with pytest.raises(NotImplementedError, match=re.escape(L.asr_strerror(N.ASR_EUNSUPPORTED).decode())):
            call()
    y = torch.zeros(2, 5, device=DEV)
    with pytest.raises(AssertionError, match=re.escape(L.asr_strerror(N.ASR_EINVAL).decode())):
        N.log_softmax_shift_bwd_split(y, nls.expand(2).contiguous(), y, 4)          # ld < C
    with pytest.raises(NotImplementedError, match=re.escape(L.asr_strerror(N.ASR_EUNSUPPORTED).decode())):
        N.log_softmax_shift_bwd_split(y, nls.expand(2).contiguous(), y, rr.SPLIT_LD_MAX + 1)
    assert L.asr_log_softmax_shift_bwd_split_bf16(None, None, None, 2, 5, None, None, 4, None, None) == N.ASR_EINVAL
    t = torch.zeros(2, 8, device=DEV)
    out = torch.zeros(8, device=DEV)
    assert L.asr_sum_leading_f32(N._p(t), 2, 6, N._p(out), N._stream()) == N.ASR_EINVAL         # n & 3


def test_empty_calls_are_ok_with_null_pointers():
    N = native()
    L = N.lib()
    s = N._stream()
    assert L.asr_log_softmax_fwd_f32(None, 0, 5, None, s) == N.ASR_OK
    assert L.asr_log_softmax_bwd_f32(None, None, 0, 5, None, s) == N.ASR_OK
    assert L.asr_sub_rowmax_f32(None, 3, 0, 5, None, None, None, None, s) == N.ASR_OK
    assert L.asr_log_softmax_shift_fwd_f32(None, 3, 0, 5, None, None, None, None, s) == N.ASR_OK
    assert L.asr_log_softmax_shift_bwd_f32(None, None, None, 0, 5, None, s) == N.ASR_OK
    assert L.asr_log_softmax_shift_bwd_split_bf16(None, None, None, 0, 5, None, None, 8, None, s) == N.ASR_OK
    assert L.asr_log_softmax_shift_bwd_split_blocks(0) == 0
    assert L.asr_argmax_rows_f32(None, 0, 5, None, s) == N.ASR_OK
    assert L.asr_split_bf16_f32(None, 0, 5, 5, None, 5, None, 5, s) == N.ASR_OK
    assert L.asr_scale_rows_f32(None, 0, 3, 5, N._p(torch.ones(3, device=DEV)), s) == N.ASR_OK


def test_sum_leading_wants_16_byte_pointers():
    """the entry refuses a pointer its float4 accesses cannot take (nothing is launched), and the
    wrapper sums such a view with torch instead"""
    N = native()
    L = N.lib()
    t = torch.zeros(3, 8, device=DEV)
    out = torch.zeros(12, device=DEV)
    p = lambda a, off: ctypes.c_void_p(a.data_ptr() + off)  # noqa: E731
    assert L.asr_sum_leading_f32(p(t, 0), 2, 8, p(out, 0), N._stream()) == N.ASR_OK
    for off in (4, 8, 12):
        assert L.asr_sum_leading_f32(p(t, off), 2, 8, p(out, 0), N._stream()) == N.ASR_EINVAL
        assert L.asr_sum_leading_f32(p(t, 0), 2, 8, p(out, off), N._stream()) == N.ASR_EINVAL
    a = rr.build('sum_leading', 'G32_n1028')['t']
    view = one_float_in(a)
    got = N.sum_leading(view)
    torch.cuda.synchronize()
    want = a.astype(np.float64).sum(0)
    bound = len(a) * 2.0 ** -24 * np.abs(a).astype(np.float64).sum(0)     # any order of fp32 adds
    assert (np.abs(host(got) - want) <= bound).all()
    assert np.array_equal(host(N.sum_leading(dev(a))), rr.ref_sum_leading(a))
