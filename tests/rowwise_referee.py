"""fp64 referees of the row-wise normaliser kernels (include/asr_amd.h; csrc/softmax.hip and
asr_scale_rows_f32 of csrc/optim.hip), one launch at a time: asr_log_softmax_{fwd,bwd}_f32,
asr_sub_rowmax_f32, asr_log_softmax_shift_{fwd,bwd}_f32, asr_log_softmax_shift_bwd_split_bf16 with
the column sums of _native.log_softmax_shift_bwd_split, asr_argmax_rows_f32, asr_sum_leading_f32,
asr_split_bf16_f32 and asr_scale_rows_f32.

Written from the header's contract; plain numpy / torch on the CPU, no native calls.  Four parts:

* `reference(op, inp)`: what a launch must leave, in fp64 or, where the contract has one correct
  answer (a single fp32 rounding, an index, a bf16 half), that answer.
* `tolerances(op, inp, want)`: per floating output, 4x the largest distance of an fp32 CPU
  evaluation of the same operation (torch ops on the same fp32 inputs, `fp32_eval`) from the fp64
  reference, plus 4 fp32 ulps (2^-23 relative) of the output's largest magnitude in its row; for
  sums, of the largest summand.  Measured per case against the reference, never against a kernel.
  One derived term is added where a one-wave sum enters (`wave_sum_term`: the row sum of dy in
  the backward kernels, the frame sums max_sum and nls_sum), for the rounding of that order.
* `judge(op, inp, got, want, tol)`: the complaints about the outputs `got` of one launch.
* `model(op, inp, mut)`: the kernels' arithmetic in numpy fp32 (lane-serial partial sums, the
  xor butterfly, exp as exp2(x log2e), log as log2(x) ln2, the grid-stride passes, the partial
  column sums and their two-stage reduction), with `mut` one wrong term.
  tests/test_rowwise_referee.py proves on the CPU that the model passes every judge at every
  case (the bounds can be met) and that each mutant is rejected at a named case.

`cases()` is the matrix: the smallest shapes that reach each code path.  One wave owns a row and
PER = ceil(C / 64) columns per lane, instantiated for PER in {1, 2, 4, 8, 16, 40, 128}: the class
edges sit on both sides of each.  The row kernels launch at most 8192 workgroups of 4 waves, the
split backward at most 2048, so a wave owns a second row from 32769 and 8193 rows on."""
import zlib

import numpy as np
import torch

F32, F64 = np.float32, np.float64
EPS32 = 2.0 ** -23
LOG2E = F32(1.4426950408889634)
LN2 = F32(0.6931471805599453)
NAN, INF = float('nan'), float('inf')
POISON = F32(-777.25)               # pre-fill of float outputs a launch must write or leave alone
POISON_I = -7                       # of int32 outputs
POISON_H = 0x5ead                   # of bf16 outputs (as bits)
SNAN = 0x7f800001                   # a signalling NaN: x * 1 would quiet it
ARG_NONE = 0x7fffffff

OPS = ('lsm_fwd', 'lsm_bwd', 'sub_rowmax', 'shift_fwd', 'shift_bwd', 'shift_bwd_split', 'argmax',
       'sum_leading', 'split_bf16', 'scale_rows')
EXACT = {'sub_rowmax': ('y', 'row_max'), 'shift_fwd': ('y',), 'argmax': ('idx',),
         'sum_leading': ('out',), 'scale_rows': ('x',), 'split_bf16': ('hi', 'lo')}
FLOATING = {'lsm_fwd': ('y',), 'lsm_bwd': ('dx',), 'sub_rowmax': ('max_sum',),
            'shift_fwd': ('nls', 'nls_sum'), 'shift_bwd': ('dx',), 'shift_bwd_split': ('dx', 'colsum')}
# outputs advertised as summed in a fixed order: two launches agree bit for bit
FIXED_ORDER = {'sub_rowmax': ('max_sum',), 'shift_fwd': ('nls_sum',), 'shift_bwd_split': ('colsum',)}

MUTANTS = ('dy_sum_drops_last_lane', 'exp_without_nls', 'nls_wrong_sign', 'mask_t_le_len',
           'lens_not_clamped', 'second_pass_dropped', 'second_pass_reuses_rows',
           'colsum_first_pass_only', 'padding_unset', 'bf16_truncates', 'lo_from_x',
           'argmax_last_tie', 'argmax_ignores_lanes', 'scale_touches_unit_rows',
           'sum_leading_skips_last')


# ------------------------------------------------------------------ bf16 halves

def f32_bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even; NaN stays NaN (quiet bit set)"""
    u = f32_bits(x).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_trunc(x):
    return (f32_bits(x) >> 16).astype(np.uint16)


def bf16_f32(h):
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def split_halves(x, rnd=bf16_rne, lo_from_x=False):
    """hi = bf16(x), lo = bf16(x - hi); x - hi is exact in fp32 for finite hi"""
    x = np.ascontiguousarray(x, dtype=F32)
    hi = rnd(x)
    with np.errstate(invalid='ignore'):
        lo = rnd(x if lo_from_x else x - bf16_f32(hi))
    return hi, lo


# ------------------------------------------------------------------ fp64 references

def _f64(a):
    return np.asarray(a, dtype=F64)


def clamp_lens(lens, T):
    return np.clip(np.asarray(lens, np.int64), 0, T)


def masked_frame_sum(v, lens):
    """sum over t < clamp(lens[b]) of v [T, B] -> [B]"""
    T = v.shape[0]
    mask = np.arange(T)[:, None] < clamp_lens(lens, T)[None, :]
    return np.where(mask, v, 0.0).sum(0)


def ref_log_softmax_fwd(x):
    """y = x - logsumexp(x, -1); an all -inf row is NaN (-inf - -inf), as in torch"""
    x = _f64(x)
    with np.errstate(invalid='ignore', divide='ignore'):
        m = x.max(-1, keepdims=True)
        return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def ref_log_softmax_bwd(y, dy):
    """dx = dy - exp(y) sum(dy, -1)"""
    y, dy = _f64(y), _f64(dy)
    return dy - np.exp(y) * dy.sum(-1, keepdims=True)


def ref_sub_rowmax(x, lens):
    """x [T, B, C] -> y = x - row_max (one fp32 rounding of the exact difference), row_max [T, B],
    max_sum [B] in fp64"""
    x = _f64(x)
    m = x.max(-1)
    with np.errstate(invalid='ignore'):
        y = (x - m[..., None]).astype(F32)
    return dict(y=y, row_max=m.astype(F32), max_sum=masked_frame_sum(m, lens))


def ref_log_softmax_shift_fwd(x, lens):
    """y = log_softmax(x) - max_c log_softmax(x) = x - max_c x (one fp32 rounding),
    nls = max_c log_softmax(x) = -log sum_c exp(x - max_c x), nls_sum [B] over t < lens[b]"""
    x = _f64(x)
    m = x.max(-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        d = x - m
        nls = -np.log(np.exp(d).sum(-1))
    return dict(y=d.astype(F32), nls=nls, nls_sum=masked_frame_sum(nls, lens))


def ref_log_softmax_shift_bwd(y, nls, dy):
    """dx = dy - exp(y + nls) sum_c dy"""
    y, nls, dy = _f64(y), _f64(nls), _f64(dy)
    return dy - np.exp(y + nls[..., None]) * dy.sum(-1, keepdims=True)


def ref_log_softmax_shift_bwd_split(y, nls, dy, ld):
    """dx as above [rows, C]; the halves of its fp32 rounding padded with zero columns to ld
    (the rule a launch is judged by is in judge(): any fp32 d within dx's tolerance may have
    been split); column sums [C]"""
    dx = ref_log_softmax_shift_bwd(y, nls, dy)
    rows, C = dx.shape
    hi = np.zeros((rows, ld), np.uint16)
    lo = np.zeros((rows, ld), np.uint16)
    hi[:, :C], lo[:, :C] = split_halves(dx.astype(F32))
    return dict(dx=dx, hi=hi, lo=lo, colsum=dx.sum(0))


def ref_argmax_rows(x):
    """index of the first maximum; a NaN entry ranks as -inf"""
    x = _f64(x)
    return np.argmax(np.where(np.isnan(x), -INF, x), -1).astype(np.int32)


def ref_sum_leading(t):
    """sum over the leading axis in that order, in fp32: the one answer of a fixed-order sum"""
    t = np.asarray(t, F32)
    out = t[0].copy()
    for g in range(1, t.shape[0]):
        out = out + t[g]
    return out


def ref_split_bf16(x):
    return split_halves(x)


def ref_scale_rows(x, scale):
    """x [T, B, C] * scale [B]: one fp32 product; factor-1 utterances keep their bits"""
    x = np.asarray(x, F32)
    sc = np.asarray(scale, F32)
    with np.errstate(invalid='ignore'):
        out = x * sc[None, :, None]
    keep = sc == 1
    out.view(np.uint32)[:, keep] = f32_bits(x)[:, keep]
    return out


def reference(op, inp):
    if op == 'lsm_fwd':
        return dict(y=ref_log_softmax_fwd(inp['x']))
    if op == 'lsm_bwd':
        return dict(dx=ref_log_softmax_bwd(inp['y'], inp['dy']))
    if op == 'sub_rowmax':
        return ref_sub_rowmax(inp['x'], inp['lens'])
    if op == 'shift_fwd':
        return ref_log_softmax_shift_fwd(inp['x'], inp['lens'])
    if op == 'shift_bwd':
        return dict(dx=ref_log_softmax_shift_bwd(inp['y'], inp['nls'], inp['dy']))
    if op == 'shift_bwd_split':
        return ref_log_softmax_shift_bwd_split(inp['y'], inp['nls'], inp['dy'], inp['ld'])
    if op == 'argmax':
        return dict(idx=ref_argmax_rows(inp['x']))
    if op == 'sum_leading':
        return dict(out=ref_sum_leading(inp['t']))
    if op == 'split_bf16':
        hi, lo = ref_split_bf16(inp['x'])
        return dict(hi=hi, lo=lo)
    if op == 'scale_rows':
        return dict(x=ref_scale_rows(inp['x'], inp['scale']))
    raise KeyError(op)


# ------------------------------------------------------------------ the fp32 yardstick

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32))


def _masked_sum32(v, lens):
    T = v.shape[0]
    mask = torch.arange(T)[:, None] < torch.from_numpy(clamp_lens(lens, T))[None, :]
    return torch.where(mask, v, torch.zeros_like(v)).sum(0)


def fp32_eval(op, inp):
    """the floating outputs of `op` from torch ops in fp32 on the CPU: every operation of the
    contract once, sums by torch.sum, the log-softmax as (x - max) - log(sum exp(x - max))"""
    if op == 'lsm_fwd':
        x = _t(inp['x'])
        d = x - x.max(-1, keepdim=True)[0]
        return dict(y=d - torch.log(torch.exp(d).sum(-1, keepdim=True)))
    if op == 'lsm_bwd':
        dy = _t(inp['dy'])
        return dict(dx=dy - torch.exp(_t(inp['y'])) * dy.sum(-1, keepdim=True))
    if op == 'sub_rowmax':
        x = _t(inp['x'])
        return dict(max_sum=_masked_sum32(x.max(-1)[0], inp['lens']))
    if op == 'shift_fwd':
        x = _t(inp['x'])
        nls = -torch.log(torch.exp(x - x.max(-1, keepdim=True)[0]).sum(-1))
        return dict(nls=nls, nls_sum=_masked_sum32(nls, inp['lens']))
    if op in ('shift_bwd', 'shift_bwd_split'):
        dy = _t(inp['dy'])
        dx = dy - torch.exp(_t(inp['y']) + _t(inp['nls'])[..., None]) * dy.sum(-1, keepdim=True)
        return dict(dx=dx) if op == 'shift_bwd' else dict(dx=dx, colsum=dx.sum(0))
    return {}


def _finite_max(a, axis=None, keepdims=False):
    a = np.abs(_f64(a))
    return np.where(np.isfinite(a), a, 0.0).max(axis=axis, keepdims=keepdims, initial=0.0)


def magnitudes(op, inp, want):
    """per floating output, the magnitude its 4 ulps are counted at: the largest of its row; for
    a sum, the largest of its summands"""
    if op in ('lsm_fwd', 'lsm_bwd', 'shift_bwd'):
        k = FLOATING[op][0]
        return {k: _finite_max(want[k], -1, True)}
    if op in ('sub_rowmax', 'shift_fwd'):
        big = _finite_max(_frame_summands(op, inp, want), 0)
        return dict(max_sum=big) if op == 'sub_rowmax' else dict(nls=np.abs(_f64(want['nls'])), nls_sum=big)
    if op == 'shift_bwd_split':
        return dict(dx=_finite_max(want['dx'], -1, True), colsum=_finite_max(want['dx'], 0))
    return {}


def _frame_summands(op, inp, want):
    """the frames that enter max_sum / nls_sum, the others 0: [T, B] in fp64"""
    v = _f64(want['row_max'] if op == 'sub_rowmax' else want['nls'])
    T = v.shape[0]
    return np.where(np.arange(T)[:, None] < clamp_lens(inp['lens'], T)[None, :], v, 0.0)


def wave_sum_term(v):
    """The rounding of a one-wave fp32 sum over the last axis of v (fp64): lane c % 64 adds its
    elements in index order, then six xor-butterfly levels add the 64 lane sums.  Every add rounds
    by at most 2^-24 of its result p_i (a lane's first element is taken, not added), so the sum
    is off by sum_i d_i p_i with |d_i| <= 2^-24: at most 2^-24 sum |p_i|, a worst case hundreds
    of times above what the order gives, and, for roundings that are independent and as often up
    as down (the usual model), beyond 6 * 2^-24 * sqrt(sum p_i^2) with probability
    2 exp(-6^2 / 2) = 3e-8 per sum (Hoeffding).  That second value is the term: the one part of
    the bound that is derived, not measured.  torch.sum adds in a cascade of its own, and its
    distance from fp64 over 5 rows of 2561 columns is by chance a fifth of what the order above
    gives (lsm_bwd/edge_C2561: 5.0x the fp32 distance, where 4x is granted)."""
    v = _f64(v)
    n = v.shape[-1]
    per = max((n + 63) // 64, 1)
    p = np.zeros(v.shape[:-1] + (per * 64,))
    p[..., :n] = np.where(np.isfinite(v), v, 0.0)
    lanes = np.cumsum(p.reshape(v.shape[:-1] + (per, 64)), -2)
    total = (lanes[..., 1:, :] ** 2).sum((-2, -1))
    level = lanes[..., -1, :]
    for half in (32, 16, 8, 4, 2, 1):
        level = level.reshape(v.shape[:-1] + (2, half)).sum(-2)
        total = total + (level ** 2).sum(-1)
    return 6 * 2.0 ** -24 * np.sqrt(total)


def derived_terms(op, inp, want):
    """what is added to the measured bound: wave_sum_term of the row sum of dy, times the
    softmax value it is multiplied with, for the three backward kernels; wave_sum_term of the
    frames for max_sum and nls_sum (max_sum_kernel is one such wave per utterance).  Nothing for
    the log-softmax values, nls and the column sums."""
    if op in ('lsm_bwd', 'shift_bwd', 'shift_bwd_split'):
        arg = _f64(inp['y']) + (_f64(inp['nls'])[..., None] if op != 'lsm_bwd' else 0.0)
        return dict(dx=wave_sum_term(inp['dy'])[..., None] * np.exp(arg))
    if op in ('sub_rowmax', 'shift_fwd'):
        k = 'max_sum' if op == 'sub_rowmax' else 'nls_sum'
        return {k: wave_sum_term(_frame_summands(op, inp, want).T)}
    return {}


def tolerances(op, inp, want):
    """-> ({output: tolerance, broadcastable to the output}, {output: the fp32 distance})"""
    f32 = fp32_eval(op, inp)
    mag = magnitudes(op, inp, want)
    extra = derived_terms(op, inp, want)
    tol, dist = {}, {}
    for k, v in f32.items():
        a, w = v.double().numpy(), _f64(want[k])
        fin = np.isfinite(w) & np.isfinite(a)
        dist[k] = float(np.abs(a[fin] - w[fin]).max(initial=0.0))
        tol[k] = 4 * dist[k] + 4 * EPS32 * mag[k] + extra.get(k, 0.0)
    return tol, dist


# ------------------------------------------------------------------ judges

def _same_bits(bad, name, got, want, payload=False):
    """bit for bit; a NaN stands for any NaN unless `payload`"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        bad.append('%s: shape %s, want %s' % (name, got.shape, want.shape))
        return
    if got.dtype.kind == 'f':
        gn, wn = np.isnan(got), np.isnan(want)
        got, want = f32_bits(got), f32_bits(want)
        if not payload:
            got, want = np.where(gn, 0x7fc00000, got), np.where(wn, 0x7fc00000, want)
    ne = got != want
    if ne.any():
        i = tuple(int(v) for v in np.argwhere(ne)[0])
        bad.append('%s: %d entries differ, first at %s: got %s want %s' % (name, int(ne.sum()), i, got[i], want[i]))


def _close(bad, stats, name, got, want, tol):
    got, want = _f64(got), _f64(want)
    if got.shape != want.shape:
        bad.append('%s: shape %s, want %s' % (name, got.shape, want.shape))
        return
    fin = np.isfinite(want)
    odd_g, odd_w = got[~fin], want[~fin]
    if not (np.array_equal(np.isnan(odd_g), np.isnan(odd_w)) and
            np.array_equal(odd_g[~np.isnan(odd_w)], odd_w[~np.isnan(odd_w)])):
        bad.append('%s: non-finite entries differ' % name)
    with np.errstate(invalid='ignore'):
        err = np.abs(got - want)
    ok = err <= np.broadcast_to(tol, want.shape)                # NaN fails
    worst = float(np.where(fin, np.nan_to_num(err, nan=INF), 0.0).max(initial=0.0))
    if stats is not None:
        with np.errstate(invalid='ignore', divide='ignore'):
            share = np.where(fin & (err > 0), np.nan_to_num(err, nan=INF) / np.broadcast_to(tol, want.shape), 0.0)
        stats[name] = worst
        stats[name + ':share'] = float(share.max(initial=0.0))     # of the bound, at the worst entry
    if not ok[fin].all():
        i = tuple(int(v) for v in np.argwhere(fin & ~ok)[0])
        bad.append('%s: error %.3g > tol %.3g at %s (worst %.3g)' % (
            name, float(np.nan_to_num(err[i], nan=INF)), float(np.broadcast_to(tol, want.shape)[i]), i, worst))


def _judge_split_halves(bad, stats, inp, got, want, tol):
    """The halves are split(d) for some fp32 d within dx's tolerance of the reference:
    |d_hat - dx| <= tol + 2^-16 |dx| with d_hat = hi + lo (what lo's rounding loses), and hi is a
    bf16 nearest to d_hat.  At an exact tie either neighbour is taken: lo = bf16_rne(d - hi)
    rounds a rest just short of half a step of hi up to the half step (0x3f817fff splits into
    0x3f81 + 2^-8), so a correct split has odd hi on a tie of d_hat.  The identity
    lo == bf16_rne(d_hat - hi) holds for every finite pair (d_hat - hi is lo); it only guards
    lo = -0 beside a nonzero sum.  Columns C .. ld-1 are +0."""
    C, ld = inp['y'].shape[-1], inp['ld']
    hi, lo = np.asarray(got['hi'], np.uint16), np.asarray(got['lo'], np.uint16)
    if hi.shape != want['hi'].shape or lo.shape != want['lo'].shape:
        bad.append('halves: shape %s / %s, want %s' % (hi.shape, lo.shape, want['hi'].shape))
        return
    if hi[:, C:].any() or lo[:, C:].any():
        bad.append('columns %d..%d are not zero: %d entries' % (C, ld - 1, int((hi[:, C:] != 0).sum() + (lo[:, C:] != 0).sum())))
    h, l = _f64(bf16_f32(hi[:, :C])), _f64(bf16_f32(lo[:, :C]))
    d_hat = h + l                                               # exact in fp64
    if not np.isfinite(d_hat).all():
        bad.append('halves: %d non-finite sums' % int((~np.isfinite(d_hat)).sum()))
        return
    _same_bits(bad, 'lo vs bf16_rne(d_hat - hi)', lo[:, :C], bf16_rne((d_hat - h).astype(F32)))
    hb = hi[:, :C].astype(np.int64)
    up, down = _f64(bf16_f32((hb + 1).astype(np.uint16))), _f64(bf16_f32((hb - 1).astype(np.uint16)))
    with np.errstate(invalid='ignore'):
        nearer = (np.abs(d_hat - up) < np.abs(l)) | (np.abs(d_hat - down) < np.abs(l))
    nearer &= (hb & 0x7fff) != 0                                # (the neighbours of +-0 are of one sign)
    if nearer.any():
        bad.append('hi is not a bf16 nearest to hi + lo at %d entries' % int(nearer.sum()))
    dx = want['dx']
    _close(bad, stats, 'dx', d_hat, dx, tol['dx'] + 2.0 ** -16 * np.abs(dx))


def judge(op, inp, got, want, tol, stats=None):
    """-> list of complaints; stats (optional dict) receives, per floating output, the worst error
    and (key + ':share') the largest share of its bound that an entry uses"""
    bad = []
    for k in EXACT.get(op, ()):
        if op == 'split_bf16':
            _judge_split_bf16(bad, k, inp, got[k], want[k])
        else:
            _same_bits(bad, k, got[k], want[k], payload=op == 'scale_rows')
    if op == 'shift_bwd_split':
        _judge_split_halves(bad, stats, inp, got, want, tol)
        _close(bad, stats, 'colsum', got['colsum'], want['colsum'], tol['colsum'])
        return bad
    for k in FLOATING.get(op, ()):
        _close(bad, stats, k, got[k], want[k], tol[k])
    return bad


def _judge_split_bf16(bad, name, inp, got, want):
    """got [rows, ld] with the columns past cols still POISON_H; NaN in, NaN out (any payload)"""
    x = np.asarray(inp['x'], F32)
    x = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x[None]
    got = np.asarray(got, np.uint16).reshape(x.shape[0], -1)
    cols = x.shape[1]
    if (got[:, cols:] != POISON_H).any():
        bad.append('%s: wrote past column %d' % (name, cols))
    g, w = got[:, :cols], np.asarray(want, np.uint16).reshape(x.shape)
    wn = np.isnan(bf16_f32(w))
    if not np.isnan(bf16_f32(g))[wn].all():
        bad.append('%s: NaN expected at %d entries' % (name, int(wn.sum())))
    _same_bits(bad, name, np.where(wn, 0, g), np.where(wn, 0, w))


# ------------------------------------------------------------------ the kernels' arithmetic in numpy fp32

def row_waves(rows):
    """waves of a launch of the one-wave-per-row kernels"""
    return int(min(max((rows + 3) // 4, 1), 8192)) * 4


def split_blocks(rows):
    return int(min(max((rows + 3) // 4, 1), 2048))


def _expf(x):
    return np.exp2(x * LOG2E)


def _logf(x):
    return np.log2(x) * LN2


def _lanes(a, fill):
    rows, C = a.shape
    per = (C + 63) // 64
    out = np.full((rows, per * 64), fill, F32)
    out[:, :C] = a
    return out.reshape(rows, per, 64)


def _lane_sum(v):
    s = np.zeros((v.shape[0], 64), F32)
    for i in range(v.shape[1]):
        s = s + v[:, i]
    return s


def _wave_sum(s, drop_last=False):
    if drop_last:
        s = s.copy()
        s[:, 63] = 0
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, 0]


def _passes(rows, nwaves, mut):
    """-> (source row of every row, rows the launch writes)"""
    src, written = np.arange(rows), np.ones(rows, bool)
    if mut == 'second_pass_dropped':
        written[nwaves:] = False
    if mut == 'second_pass_reuses_rows':
        src = src % nwaves
    return src, written


def _finish(out, written, fill):
    out = np.array(out, copy=True)
    out[~written] = fill
    return out


def _model_frame_sum(v, lens, mut):
    """max_sum_kernel: lane t % 64 adds frames t, t + 64, .. in order, then the butterfly.
    Memory past the T frames reads as POISON (the mutants that run past it)"""
    T, B = v.shape
    mem = np.concatenate([v, np.full((8, B), POISON, F32)], 0)
    out = np.zeros(B, F32)
    for b in range(B):
        n = int(lens[b])
        if mut != 'lens_not_clamped':
            n = min(max(n, 0), T)
        if mut == 'mask_t_le_len':
            n += 1
        n = min(max(n, 0), T + 8)
        part = np.zeros((1, ((n + 63) // 64) * 64 or 64), F32)
        part[0, :n] = mem[:n, b]
        out[b] = _wave_sum(_lane_sum(part.reshape(1, -1, 64)))[0]
    return out


def _model_dx(y, nls, dy, mut):
    """dy - exp(y [+ nls]) * sum(dy) per row, in the kernels' order"""
    vy, vg = _lanes(y, -INF), _lanes(dy, 0.0)
    s = _wave_sum(_lane_sum(vg), mut == 'dy_sum_drops_last_lane')
    arg = vy if nls is None or mut == 'exp_without_nls' else vy + nls[:, None, None]
    d = vg - _expf(arg) * s[:, None, None]
    return d.reshape(y.shape[0], -1)[:, :y.shape[1]]


def model(op, inp, mut=None):
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        return _model(op, inp, mut)


def _model(op, inp, mut):
    rnd = bf16_trunc if mut == 'bf16_truncates' else bf16_rne
    if op in ('lsm_fwd', 'sub_rowmax', 'shift_fwd'):
        x = np.asarray(inp['x'], F32)
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        src, written = _passes(x2.shape[0], row_waves(x2.shape[0]), mut)
        v = _lanes(x2[src], -INF)
        m = v.max((1, 2)) if v.shape[0] else np.zeros(0, F32)
        if op == 'sub_rowmax':
            y = (x2[src] - m[:, None]).astype(F32)
            rm = _finish(m, written, POISON).reshape(shape[:2])
            return dict(y=_finish(y, written, POISON).reshape(shape), row_max=rm,
                        max_sum=_model_frame_sum(rm, inp['lens'], mut))
        s = _wave_sum(_lane_sum(_expf(v - m[:, None, None])))
        if op == 'lsm_fwd':
            y = ((v - m[:, None, None]) - _logf(s)[:, None, None]).reshape(x2.shape[0], -1)[:, :shape[-1]]
            return dict(y=_finish(y, written, POISON).reshape(shape))
        nls = _logf(s) if mut == 'nls_wrong_sign' else -_logf(s)
        nls = _finish(nls, written, POISON).reshape(shape[:2])
        y = (x2[src] - m[:, None]).astype(F32)
        return dict(y=_finish(y, written, POISON).reshape(shape), nls=nls,
                    nls_sum=_model_frame_sum(nls, inp['lens'], mut))
    if op in ('lsm_bwd', 'shift_bwd', 'shift_bwd_split'):
        y, dy = np.asarray(inp['y'], F32), np.asarray(inp['dy'], F32)
        rows, C = y.shape
        nls = np.asarray(inp['nls'], F32) if op != 'lsm_bwd' else None
        nwaves = split_blocks(rows) * 4 if op == 'shift_bwd_split' else row_waves(rows)
        src, written = _passes(rows, nwaves, mut)
        d = _model_dx(y[src], None if nls is None else nls[src], dy[src], mut)
        if op != 'shift_bwd_split':
            return dict(dx=_finish(d, written, POISON))
        ld = inp['ld']
        dp = np.zeros((rows, ld), F32)
        dp[:, :C] = d
        hi, lo = split_halves(dp, rnd, mut == 'lo_from_x')
        hi, lo = _finish(hi, written, POISON_H), _finish(lo, written, POISON_H)
        if mut == 'padding_unset':
            hi[:, C:], lo[:, C:] = POISON_H, POISON_H
        # cs[]: every wave adds its rows in order; one partial row per workgroup
        npass = (rows + nwaves - 1) // nwaves
        if mut in ('colsum_first_pass_only', 'second_pass_dropped'):
            npass = 1
        acc = np.zeros((npass * nwaves, ld), F32)
        n = min(rows, npass * nwaves)
        acc[:n] = dp[:n]
        cs = np.zeros((nwaves, ld), F32)
        for p in range(npass):
            cs = cs + acc[p * nwaves:(p + 1) * nwaves]
        w = cs.reshape(-1, 4, ld)
        part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
        nb = part.shape[0]
        if nb % 32 == 0 and nb > 32:        # the two stages of _native.log_softmax_shift_bwd_split
            part = ref_sum_leading(part.reshape(32, -1)).reshape(nb // 32, ld)
        return dict(hi=hi, lo=lo, colsum=ref_sum_leading(part)[:C])
    if op == 'argmax':
        x = np.asarray(inp['x'], F32)
        rows, C = x.shape
        src, written = _passes(rows, row_waves(rows), mut)
        v = np.where(np.isnan(x[src]), F32(-INF), x[src])
        if mut == 'argmax_ignores_lanes':
            idx = np.full(rows, ARG_NONE, np.int32)
            live = np.arange(C) % 64 < C % 64
            if live.any():
                idx = np.flatnonzero(live)[np.argmax(v[:, live], -1)].astype(np.int32)
        elif mut == 'argmax_last_tie':
            idx = (C - 1 - np.argmax(v[:, ::-1], -1)).astype(np.int32)
        else:
            idx = np.argmax(v, -1).astype(np.int32)
        return dict(idx=_finish(idx, written, POISON_I))
    if op == 'sum_leading':
        t = np.asarray(inp['t'], F32)
        return dict(out=ref_sum_leading(t[:-1] if mut == 'sum_leading_skips_last' and len(t) > 1 else t))
    if op == 'split_bf16':
        x = np.asarray(inp['x'], F32)
        x2 = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x[None]
        hi, lo = split_halves(x2, rnd, mut == 'lo_from_x')
        pad = np.full((x2.shape[0], inp.get('gap', 0)), POISON_H, np.uint16)
        return dict(hi=np.concatenate([hi, pad], 1), lo=np.concatenate([lo, pad], 1))
    if op == 'scale_rows':
        x, sc = np.asarray(inp['x'], F32), np.asarray(inp['scale'], F32)
        if mut == 'scale_touches_unit_rows':
            return dict(x=x * sc[None, :, None])
        return dict(x=ref_scale_rows(x, sc))
    raise KeyError(op)


# ------------------------------------------------------------------ the case matrix

CLASS_EDGES = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2401, 2560, 2561, 5000, 8192)
FAMILY_C = (7, 130, 2401)
X_FAMILIES = ('randn4', 'peaked', 'masked', 'constant', 'offset1e4', 'randn30')
DY_FAMILIES = ('randn', 'posterior', 'one_hot', 'zero', 'zero_row_sums')
STRIDE_ROWS, STRIDE_C = 32771, 3                # one row-kernel wave owns rows r and r + 32768
SPLIT_STRIDE_ROWS, SPLIT_STRIDE_C, SPLIT_STRIDE_LD = 8197, 5, 8
SPLIT_LD_MAX = 2560
LENS_T = (1, 63, 64, 65, 130)
UNSUPPORTED_C = 8193


def edge_rows(C):
    return 5 if C > 1024 else 67


def _rng(op, name):
    return np.random.default_rng(zlib.crc32(('%s/%s' % (op, name)).encode()))


def x_family(kind, rows, C, rng):
    x = rng.standard_normal((rows, C)).astype(F32)
    if kind == 'randn4':
        x *= 4
    elif kind == 'peaked':                      # exp(-40 + 8) C < 2^-24: the sum is exactly 1
        x[np.arange(rows), rng.integers(0, C, rows)] += 40
    elif kind == 'masked':
        x *= 4
        gone = rng.random((rows, C)) < 1 / 3
        gone[np.arange(rows), rng.integers(0, C, rows)] = False     # never the whole row
        x[gone] = -INF
    elif kind == 'constant':
        x[:] = (np.arange(rows, dtype=F32) * 1.75 - 2.5)[:, None]
    elif kind == 'offset1e4':
        x = (x * 4 + F32(1e4)).astype(F32)
    elif kind == 'randn30':
        x *= 30
    else:
        raise KeyError(kind)
    return x


def dy_family(kind, rows, C, rng):
    if kind == 'randn':
        return rng.standard_normal((rows, C)).astype(F32)
    if kind == 'posterior':
        e = np.exp(2 * rng.standard_normal((rows, C)))
        return (e / e.sum(-1, keepdims=True)).astype(F32)
    dy = np.zeros((rows, C), F32)
    if kind == 'one_hot':
        dy[np.arange(rows), rng.integers(0, C, rows)] = 1
    elif kind == 'zero_row_sums':               # small integers in pairs: every partial sum is exact
        k = rng.integers(1, 64, (rows, C // 2)).astype(F32)
        dy[:, :C // 2], dy[:, C // 2:2 * (C // 2)] = k, -k
        dy = rng.permuted(dy, axis=1)
    elif kind != 'zero':
        raise KeyError(kind)
    return dy


def _bwd_inputs(op, x, dy, ld=None):
    """the backward kernels read what the forward ones wrote: the reference's outputs in fp32"""
    if op == 'lsm_bwd':
        with np.errstate(invalid='ignore'):
            return dict(y=ref_log_softmax_fwd(x).astype(F32), dy=dy)
    f = ref_log_softmax_shift_fwd(x[:, None, :], np.zeros(1, np.int32))
    inp = dict(y=f['y'][:, 0], nls=f['nls'][:, 0].astype(F32), dy=dy)
    if ld is not None:
        inp['ld'] = ld
    return inp


def _up(n, k):
    return (n + k - 1) // k * k


def _tbc(x, lens):
    return dict(x=x[:, None, :] if x.ndim == 2 else x, lens=np.asarray(lens, np.int32))


def _lens_for(T, B):
    return [0, T, T + 3, -2, max(T // 2, 1)][:B] if B > 1 else None


def _build_row_op(op, kind, rows, C, dykind='randn', ld=None, name=''):
    rng = _rng(op, name)
    x = x_family(kind, rows, C, rng)
    if op in ('lsm_fwd', 'argmax'):
        return dict(x=x)
    if op in ('sub_rowmax', 'shift_fwd'):
        return _tbc(x, [rows - rows // 3])
    return _bwd_inputs(op, x, dy_family(dykind, rows, C, rng), ld)


ROW_OPS = ('lsm_fwd', 'lsm_bwd', 'sub_rowmax', 'shift_fwd', 'shift_bwd', 'argmax')


def _argmax_specials():
    def rows_of(C, pairs):
        x = np.full((len(pairs), C), -1.0, F32)
        for r, cols in enumerate(pairs):
            x[r, list(cols)] = 2.0
        return x
    sp = {
        'tie_c_c64': rows_of(200, [(5, 69), (69, 5 + 128), (1, 65, 129), (63, 127), (133, 197)]),
        'tie_c_c1': rows_of(130, [(10, 11), (63, 64), (127, 128), (128, 129)]),
        'tie_all_lanes_64': np.full((3, 64), 0.5, F32),
        'tie_all_lanes_130': np.full((3, 130), -3.0, F32),
        'all_minus_inf': np.full((2, 65), -INF, F32),
        'c1': np.array([[3.0], [-INF], [0.0]], F32),
    }
    for C in (2, 63, 64, 65, 130):
        sp['max_in_last_column_%d' % C] = rows_of(C, [(C - 1,)])
    # a NaN ranks as -inf, wherever it sits: alone in its lane's first column, in a lane whose
    # partner holds the maximum, in a second column, and in a row of nothing else
    nan = rows_of(130, [(37,), (100,), (3,), (64,)])
    nan[0, 5], nan[1, 0], nan[2, 64 + 3], nan[3, 64] = NAN, NAN, NAN, NAN
    nan[3, :64] = NAN
    sp['nan_ranks_as_minus_inf'] = nan
    sp['all_nan'] = np.full((2, 7), NAN, F32)
    return sp


def _coarse(op, C):
    """integers in [-3, 3]: ties in every row"""
    return _rng(op, 'coarse%d' % C).integers(-3, 4, (67, C)).astype(F32)


def _split_specials():
    def bits(*u):
        return np.array(u, np.uint32).view(F32)
    return np.concatenate([
        bits(0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0xbf808000, 0xbf818000,   # ties: to even
             0x7f7f8000, 0x7f7f7fff, 0x00008000, 0x00018000),                         # to inf; denormal ties
        bits(0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00012345, 0x00800000),
        bits(0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff),                          # NaN
        bits(0x7f800000, 0xff800000),                                                  # +-inf
        np.array([1.0, -1.0, 3.14159274, 1e-30, -6.5e37, 257.0], F32)])


def cases():
    """-> [(op, name)], every case of the matrix; build(op, name) makes its inputs"""
    out = []
    for op in ROW_OPS:
        out += [(op, 'edge_C%d' % C) for C in CLASS_EDGES]
        out.append((op, 'stride_%dx%d' % (STRIDE_ROWS, STRIDE_C)))
    for C in CLASS_EDGES:
        out += [('shift_bwd_split', 'edge_C%d_ld%d' % (C, ld))
                for ld in sorted({C, _up(C, 8), _up(C, 64)}) if ld <= SPLIT_LD_MAX]
    out += [('shift_bwd_split', n) for n in (
        'next_class_C120_ld192', 'stride_%dx%d_ld%d' % (SPLIT_STRIDE_ROWS, SPLIT_STRIDE_C, SPLIT_STRIDE_LD),
        'blocks31', 'blocks32', 'blocks33', 'blocks64', 'blocks64_ld7', 'blocks2048')]
    for op in ('lsm_fwd', 'sub_rowmax', 'shift_fwd', 'lsm_bwd', 'shift_bwd', 'shift_bwd_split'):
        out += [(op, '%s_C%d' % (k, C)) for k in X_FAMILIES for C in FAMILY_C]
    for op in ('lsm_bwd', 'shift_bwd', 'shift_bwd_split'):
        out += [(op, 'dy_%s_C%d' % (k, C)) for k in DY_FAMILIES[1:] for C in FAMILY_C]
    for op in ('lsm_fwd', 'sub_rowmax', 'shift_fwd'):
        out.append((op, 'one_row_all_minus_inf'))
    for op in ('sub_rowmax', 'shift_fwd'):
        out += [(op, 'lens_T%d_B5' % T) for T in LENS_T]
        out += [(op, 'lens_T%d_B1_len%d' % (T, n)) for T in LENS_T for n in (0, T, T + 3, -2)]
        out.append((op, 'lens_T0_B5'))
    out += [('argmax', n) for n in _argmax_specials()]
    out += [('argmax', 'coarse_C%d' % C) for C in (63, 64, 65, 130, 200)]
    out += [('sum_leading', 'G%d_n%d' % (G, n)) for G in (1, 2, 32, 64) for n in (4, 1020, 1024, 1028)]
    out += [('split_bf16', n) for n in (
        'specials', 'specials_tail3', 'dense_5x2401', 'dense_3x7', 'dense_67x130', 'dense_4x1024',
        'halves_of_concat_5x130', 'halves_of_concat_4x64', 'strided_x_5x130', 'strided_x_9x5',
        'offset4_flat_1027', 'offset4_7x130', 'offset4_4x64')]
    out += [('scale_rows', 'T%d_C%d' % (T, C)) for T in (1, 7, 8, 9) for C in (1, 256, 257)]
    return out


def build(op, name):
    """the inputs of a case: numpy arrays (and ints), made from the name alone"""
    rng = _rng(op, name)
    parts = name.split('_')
    if op == 'shift_bwd_split':
        if name.startswith('edge_'):
            C, ld = int(parts[1][1:]), int(parts[2][2:])
            return _build_row_op(op, 'randn4', edge_rows(C), C, ld=ld, name=name)
        if name.startswith('next_class'):
            return _build_row_op(op, 'randn4', 19, 120, ld=192, name=name)
        if name.startswith('stride_'):
            return _build_row_op(op, 'randn4', SPLIT_STRIDE_ROWS, SPLIT_STRIDE_C, ld=SPLIT_STRIDE_LD, name=name)
        if name.startswith('blocks'):
            nb = int(parts[0][6:])
            rows = {31: 124, 32: 126, 33: 129, 64: 256, 2048: 8192}[nb]
            assert split_blocks(rows) == nb
            return _build_row_op(op, 'randn4', rows, 5, ld=7 if name.endswith('ld7') else 8, name=name)
    if op in ROW_OPS + ('shift_bwd_split',):
        if name.startswith('edge_'):
            C = int(parts[1][1:])
            return _build_row_op(op, 'randn4', edge_rows(C), C, name=name)
        if name.startswith('stride_'):
            return _build_row_op(op, 'randn4', STRIDE_ROWS, STRIDE_C, name=name)
        if name == 'one_row_all_minus_inf':
            x = x_family('randn4', 3, 70, rng)
            x[1] = -INF
            return dict(x=x) if op == 'lsm_fwd' else _tbc(x, [3])
        if name.startswith('lens_'):
            T, B = int(parts[1][1:]), int(parts[2][1:])
            lens = _lens_for(T, B) or [int(parts[3][3:])]
            return _tbc(x_family('randn4', T * B, 9, rng).reshape(T, B, 9), lens)
        if name.startswith('dy_'):
            C = int(parts[-1][1:])
            ld = _up(C, 8) if op == 'shift_bwd_split' else None
            return _build_row_op(op, 'randn4', 5 if C > 1024 else 19, C, '_'.join(parts[1:-1]), ld, name)
        if name.startswith('coarse_'):
            return dict(x=_coarse(op, int(parts[1][1:])))
        if op == 'argmax' and name in _argmax_specials():
            return dict(x=_argmax_specials()[name])
        kind, C = '_'.join(parts[:-1]), int(parts[-1][1:])
        ld = _up(C, 8) if op == 'shift_bwd_split' else None
        return _build_row_op(op, kind, 5 if C > 1024 else 19, C, ld=ld, name=name)
    if op == 'sum_leading':
        G, n = int(parts[0][1:]), int(parts[1][1:])
        return dict(t=(rng.standard_normal((G, n)) * 4).astype(F32))
    if op == 'scale_rows':
        T, C = int(parts[0][1:]), int(parts[1][1:])
        x = (rng.standard_normal((T, 5, C)) * 4).astype(F32)
        # what x * 1 would change sits in the factor-1 utterances: a signalling NaN, and -0 with them
        xb = x.view(np.uint32)
        xb[T - 1, 0, C - 1] = 0xffc12345
        xb[0, 0, 0] = SNAN
        x[T // 2, 1, C // 2], x[0, 3, 0], x[T - 1, 4, C - 1] = -0.0, -0.0, -3.0
        return dict(x=x, scale=np.array([1, 1, -0.5, 3, 0], F32))
    if op == 'split_bf16':
        sp = _split_specials()
        if name == 'specials':                  # one contiguous row of 4 k elements
            return dict(x=np.concatenate([sp, np.ones(-len(sp) % 4, F32)]), mode='contiguous')
        if name == 'specials_tail3':
            return dict(x=np.concatenate([sp, np.ones(-len(sp) % 4 + 3, F32)]), mode='contiguous')
        r, c = (int(v) for v in parts[-1].split('x')) if 'x' in parts[-1] else (1, int(parts[-1]))
        x = (rng.standard_normal((r, c)) * np.exp(3 * rng.standard_normal((r, c)))).astype(F32)
        x.reshape(-1)[:len(sp)] = sp[:x.size]
        if name.startswith('dense'):            # [rows, cols] contiguous, dense outputs
            return dict(x=x, mode='dense')
        if name.startswith('halves'):           # outputs are column blocks of one [rows, 3 cols]
            return dict(x=x, mode='dense', gap=2 * c)
        if name.startswith('strided_x'):        # x is a column block of a wider tensor
            return dict(x=x, mode='strided_x', xgap=3, gap=1)
        if r == 1:
            return dict(x=x[0], mode='offset4')
        return dict(x=x, mode='offset4')        # a contiguous view one float into its allocation
    raise KeyError((op, name))

