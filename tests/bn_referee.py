"""fp64 referee of the fused BatchNorm2d + Hardtanh kernels (csrc/bnact.hip) behind
asr_bn_act_fwd_f32, asr_bn_act_bwd_f32 and asr_bn_act_bwd_phase_f32, one launch at a time.

Written from the contract in include/asr_amd.h; plain numpy / torch on the CPU, no native calls.
Every array of a case is held in LOGICAL order [B, C, H, W]; `to_storage` / `from_storage` are the
three storage orders of the ABI (NCHW, channels-last [B, H, W, C], time-major [H, B, C, W]).

* `reference(op, inp)`, op in OPS = fwd, bwd, bwd_phase1, bwd_phase2: in fp64, what the launch
  must leave.  fwd: out, save_mean, save_invstd and the running statistics after the call
  (momentum, unbiased variance, variance itself at n = 1); from `chan_sums` ([2][C] sums of the
  bias-free input) when the case hands them over, the bias then shifting the mean only.  bwd: dx,
  dgamma, dbeta, dconv_bias and the workspace sums (2 C interleaved doubles: sum dy', sum dy' xhat)
  from the case's fp32 save_mean / save_invstd; phase 2 takes dx from the sums and n_total the case
  supplies.  The mask is torch's hardtanh_backward: dy passes where lo < y < hi strictly (not at a
  NaN); Hardtanh itself lets a NaN through.
* `tolerances(op, inp, want)`: derived below, nothing fitted to a kernel.
* `judge(op, inp, got, want, tol)`: the complaints about one launch on POISONed outputs.
* `model(op, inp, mut)`: the kernels' arithmetic in numpy fp32 with the partial sums in the
  kernels' order, `mut` one wrong term (MUTANTS).  tests/test_bn_referee.py proves that the model
  passes every judge and that every mutant is rejected at a named case.
* `exact_case`: eval mode, eps = 0, running_var in {0.25, 1, 4}, integer running_mean / beta /
  conv_bias, gamma a power of two, small-integer x and dy: every product and partial sum is exact
  in fp32 in any order and every output is compared with equality, so every index, tile, tail and
  transposition is pinned, and so is the strict inequality at both clamps (many y equal lo and hi).
* `families(spec)`: the kernel instantiations the launchers select for a case (a table kept here
  from the launchers' conditions); ALL_FAMILIES is everything they can select.

Tolerances.  u = 2^-23.  An elementwise fp32 step costs u |result|.  A sum of fp32 terms costs
depth u sum|terms|, depth being the fp32 summation depth of the path (`depth`): the serial terms
of a thread + the serial LDS column terms + the tree levels of block_sum; across workgroups the
sum is an atomic double and costs nothing.  From the launch geometry (P = B H W pixels, 256
threads a workgroup):

    nchw    one workgroup a (b, c) plane: ceil(HW / 256) serial terms, 6 butterfly levels of the
            wave sum, 3 serial adds over the four waves
    nhwc4   W = clamp(P / 64, 1, 4096) workgroups own ceil(P / W) consecutive pixels each, a thread
            4 channels of every PL-th pixel (PL = 1024 / C): ceil(ceil(P / W) / PL) serial terms,
            then PL serial LDS column terms
    nhwc8   the same workgroups stride over chunks of 2 PL pixels (PL = 2048 / C), two terms a
            trip: 2 ceil(P / (2 PL W)) serial terms, then PL column terms
    tm      min(ceil(B H / R), 2048) workgroups stride over tiles of R rows of W pixels
            (R = min(8, 12288 / (C W))): trips ceil(R W / PL) serial terms, then PL column terms

Forward, training, own statistics (the sums are taken about a per-channel pivot pv, an element of
the channel, bias-free): with dev = |v - mean|, mad its mean and maxdev its maximum,
    d mean   = (depth + 1) u (mad + maxdev) + u |mean|          (|v - pv| <= dev + maxdev)
    d var    = (depth + 3) u (var + maxdev^2)                    (mean of (v - pv)^2 <= var + maxdev^2;
                                                                  + 3: the roundings of v - pv and its square)
which is the bound of a centred evaluation about ANY element of the channel and does not grow
with mean / std; with chan_sums both are double arithmetic on the caller's sums (u |mean| only).
    d invstd = invstd^3 d var / 2 + u invstd;    eval mode: 3 u invstd (add, sqrt, divide), d mean 0
    d y      = |gamma| dev d invstd + |gamma invstd| d mean
               + u (|x sc| + 2 |m' sc| + |sh| + |y|),  sc = gamma invstd, m' = mean - bias, sh = beta - m' sc
(the kernels evaluate fma(x, sc, sh): roundings of sc, m', m' sc, sh and the fma).  out must lie
between clamp(y - d y) and clamp(y + d y); a bf16 out between the bf16 roundings (nearest even) of
these two, so where y sits within d y of a rounding boundary either neighbour is accepted.
Running statistics: momentum times the above + 3 u of the terms.

Backward (save_mean / save_invstd are inputs): xhat = (x - m') invstd costs
e_xh = u (|m'| invstd + 2 |xhat|), y = fma(xhat, gamma, beta) costs e_y = |gamma| e_xh + u |y|.
An element with |y - lo| <= e_y or |y - hi| <= e_y may take either side of the mask: it is left out
of the dx comparison and widens the sum tolerances by |dy| and |dy xhat|.  CAP: at most 1 element in
1000 (rounded up) may be left out, else the case fails.
    d s1 = depth u sum|dy'| (+ left out);   d s2 = (depth + 1) u sum|dy' xhat| + sum|dy'| e_xh (+ left out)
    dbeta, dgamma: + u |s|;   dconv_bias (eval) = gamma invstd s1: |gamma invstd| d s1 + 3 u |.|
    k_i = s_i / n: d k_i = d s_i / n + u |k_i| (phase 2: the caller's sums, d s_i = 0)
    d dx = |gamma invstd| (d k1 + |xhat| d k2 + e_xh |k2| + u (|xhat k2| + |dy' - k1| + |inner|)) + 2 u |dx|
A bf16 dx (bf16 x) is held like a bf16 out.
"""
import zlib

import numpy as np

from rowwise_referee import bf16_f32, bf16_rne, bf16_trunc

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
NAN = float('nan')
POISON = F32(-776.0)                # pre-fill of every output (exact in bf16 too)
CAP = 1000                          # at most 1 element in CAP (rounded up) left out near a clamp
EPS, MOMENTUM = 1e-5, 0.1
OPS = ('fwd', 'bwd', 'bwd_phase1', 'bwd_phase2')
MUTANTS = ('mask_le_hi', 'mask_ge_lo', 'slice_last_pixel_dropped', 'second_trip_dropped',
           'tile_row_from_wrong_batch', 'channels_ge_256_missing', 'biased_running_var',
           'bias_missing_from_mean', 'k2_dropped', 'bf16_truncates', 'nan_clamped_to_lo',
           'tm_index_b_h_swapped')


# ------------------------------------------------------------------ storage orders

def to_storage(a, layout):
    """logical [B, C, H, W] -> the flat buffer of `layout` (nchw | nhwc | tm)"""
    perm = {'nchw': (0, 1, 2, 3), 'nhwc': (0, 2, 3, 1), 'tm': (2, 0, 1, 3)}[layout]
    return np.ascontiguousarray(np.transpose(a, perm)).reshape(-1)


def from_storage(flat, shape, layout):
    B, C, H, W = shape
    if layout == 'nchw':
        return flat.reshape(B, C, H, W)
    if layout == 'nhwc':
        return flat.reshape(B, H, W, C).transpose(0, 3, 1, 2)
    return flat.reshape(H, B, C, W).transpose(1, 2, 0, 3)


def layouts(spec):
    """(x and dx, out or dy) storage orders"""
    xl = 'nhwc' if spec['cl'] else 'nchw'
    return xl, ('tm' if spec['tm'] else xl)


# ------------------------------------------------------------------ launch geometry

def nwg(P):
    return int(min(max(P // 64, 1), 4096))


def tm_rows(cw):
    return min(8, 48 * 1024 // (cw * 4))


def stats_path(spec):
    return 'nhwc4' if spec['cl'] else 'nchw'


def apply_path(spec):
    """kernel family of the forward apply pass / of both backward passes"""
    if not spec['cl']:
        return 'nchw'
    C, W = spec['C'], spec['W']
    if spec['tm'] and C * W % 8 == 0 and tm_rows(C * W) >= 1:
        return 'tm'
    if not spec['tm'] and spec['x_bf16'] and C % 8 == 0 and 256 % (C // 8) == 0:
        return 'nhwc8'
    return 'nhwc4'


def depth(path, spec):
    B, C, H, W = (spec[k] for k in 'BCHW')
    P = B * H * W
    if path == 'nchw':
        return -(-H * W // 256) + 6 + 3
    if path == 'nhwc4':
        PL, per = 1024 // C, -(-P // nwg(P))
        return -(-per // PL) + PL
    if path == 'nhwc8':
        PL = 2048 // C
        return 2 * -(-P // (2 * PL * nwg(P))) + PL
    R, PL = tm_rows(C * W), 1024 // C
    tiles = -(-B * H // R)
    return -(-tiles // min(tiles, 2048)) * -(-R * W // PL) + PL


def _t(bf16):
    return 'bf16' if bf16 else 'f32'


def families(spec):
    """the kernels one launch of the case runs, as the launchers of csrc/bnact.hip select them"""
    op, xt, ot, tm = spec['op'], _t(spec['x_bf16']), _t(spec['o_bf16']), int(spec['tm'])
    path = apply_path(spec)
    if op == 'fwd':
        if not spec['training']:
            out = ['eval_stats']
        elif spec['chan_sums']:
            out = ['finalize_from_sums']
        else:
            out = ['zero_doubles', 'finalize',
                   'stats_nhwc<%s>' % xt if spec['cl'] else 'stats_nchw']
        out.append({'nchw': 'fwd_nchw<%s,%d>' % (ot, tm), 'tm': 'fwd_tm<%s,%s>' % (xt, ot),
                    'nhwc8': 'fwd_nhwc8<bf16,%s>' % ot, 'nhwc4': 'fwd_nhwc<%s,%s,%d>' % (xt, ot, tm)}[path])
        return out
    names = {'nchw': ('bwd_reduce_nchw<%s,%d>' % (ot, tm), 'bwd_apply_nchw<%s,%d>' % (ot, tm)),
             'tm': ('bwd_tm<%s,%s,0>' % (xt, ot), 'bwd_tm<%s,%s,1>' % (xt, ot)),
             'nhwc8': ('bwd_nhwc8<bf16,%s,0>' % ot, 'bwd_nhwc8<bf16,%s,1>' % ot),
             'nhwc4': ('bwd_reduce_nhwc<%s,%s,%d>' % (xt, ot, tm), 'bwd_apply_nhwc<%s,%s,%d>' % (xt, ot, tm))}[path]
    out = []
    if op != 'bwd_phase2':
        out += ['zero_doubles', names[0], 'param_grads']
    if op != 'bwd_phase1':
        out.append(names[1])
    return out


def _all_families():
    T, out = ('f32', 'bf16'), {'eval_stats', 'finalize_from_sums', 'zero_doubles', 'finalize', 'stats_nchw',
                               'stats_nhwc<f32>', 'stats_nhwc<bf16>', 'param_grads'}
    for ot in T:
        out |= {'fwd_nhwc8<bf16,%s>' % ot, 'bwd_nhwc8<bf16,%s,0>' % ot, 'bwd_nhwc8<bf16,%s,1>' % ot}
        for tm in (0, 1):
            out |= {'fwd_nchw<%s,%d>' % (ot, tm), 'bwd_reduce_nchw<%s,%d>' % (ot, tm),
                    'bwd_apply_nchw<%s,%d>' % (ot, tm)}
        for xt in T:
            out |= {'fwd_tm<%s,%s>' % (xt, ot), 'bwd_tm<%s,%s,0>' % (xt, ot), 'bwd_tm<%s,%s,1>' % (xt, ot)}
            for tm in (0, 1):
                out |= {'fwd_nhwc<%s,%s,%d>' % (xt, ot, tm), 'bwd_reduce_nhwc<%s,%s,%d>' % (xt, ot, tm),
                        'bwd_apply_nhwc<%s,%s,%d>' % (xt, ot, tm)}
    return out


ALL_FAMILIES = _all_families()


# ------------------------------------------------------------------ the matrix

SPECS = {}
DEFAULTS = dict(cl=False, x_bf16=False, o_bf16=False, tm=False, training=True, bias=False,
                chan_sums=False, null_running=False, lo=0.0, hi=20.0, kind='randn', via='abi')


def _add(ops, tag, B, C, H, W, **kw):
    for op in ops.split():
        s = dict(DEFAULTS, op=op, B=B, C=C, H=H, W=W, **kw)
        if op != 'fwd':
            s['chan_sums'] = s['null_running'] = False
        name = '%s/%s_B%dC%dH%dW%d' % (op, tag, B, C, H, W)
        assert name not in SPECS, name
        SPECS[name] = dict(s, name=name)


def _matrix():
    FB, ALL = 'fwd bwd', 'fwd bwd bwd_phase1 bwd_phase2'
    dt = lambda o: 'o' + _t(o)  # noqa: E731
    # --- NCHW planes: every out / dy type and order at HW < 256; HW > 256 and no multiple of it
    _add(FB, 'nchw_n1', 1, 1, 1, 1)                                  # n = 1: var 0, running_var takes var
    for o in (False, True):
        for tm in (False, True):
            _add(FB, 'nchw_%s_tm%d' % (dt(o), tm), 2, 3, 5, 7, o_bf16=o, tm=tm)
    _add(ALL, 'nchw_bias_tm', 3, 3, 9, 37, tm=True, bias=True)       # HW = 333
    _add(FB, 'nchw_eval_bias', 3, 3, 9, 37, training=False, bias=True)
    _add(FB, 'nchw_eval_tm_obf16', 2, 1, 3, 90, training=False, tm=True, o_bf16=True)    # HW = 270
    _add(FB, 'nchw_w1', 5, 3, 3, 1)
    _add('fwd', 'nchw_chan_sums_bias', 3, 3, 9, 37, chan_sums=True, bias=True)
    _add('fwd', 'nchw_null_running', 2, 3, 5, 7, null_running=True)
    _add(FB, 'nchw_lohi', 3, 3, 9, 37, lo=-1.5, hi=2.25)
    for C in (6, 12):            # the wrapper takes channels-last storage of these down the NCHW path
        _add(FB, 'wrapper_cl', 2, C, 4, 5, via='wrapper', cl_storage=True)
    # --- channels-last, 4 channels a thread: every supported C; P = 165 is no multiple of PL, 2 PL,
    # 4 PL for any of them and two workgroups own 83 and 82 pixels
    for C in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        _add(FB, 'nhwc4', 3, C, 5, 11, cl=True)
    _add(FB, 'nhwc4_h1_over_wg', 3, 32, 1, 43, cl=True)              # P = 129 = 2 * 64 + 1, H = 1
    _add(FB, 'nhwc4_one_wg', 1, 16, 3, 5, cl=True)                   # P = 15
    _add(FB, 'nhwc4_p1', 1, 4, 1, 1, cl=True)
    _add(FB, 'nhwc4_eval_bias', 3, 32, 5, 11, cl=True, training=False, bias=True)
    _add(ALL, 'nhwc4_bias', 3, 64, 5, 11, cl=True, bias=True)
    _add('fwd', 'nhwc4_chan_sums', 3, 32, 5, 11, cl=True, chan_sums=True)
    _add('fwd', 'nhwc4_null_running', 3, 32, 5, 11, cl=True, null_running=True)
    _add(FB, 'nhwc4_lohi', 3, 16, 5, 11, cl=True, lo=-1.5, hi=2.25, bias=True)
    # every type of x, of out / dy and both orders at C = 4, W odd (C W % 8 != 0: element-wise time-major)
    for xb in (False, True):
        for o in (False, True):
            for tm in (False, True):
                _add(FB, 'nhwc4_x%s_%s_tm%d' % (_t(xb), dt(o), tm), 3, 4, 7, 5, cl=True, x_bf16=xb, o_bf16=o, tm=tm)
    _add(FB, 'nhwc4_tm_wide', 2, 1024, 3, 13, cl=True, tm=True)     # C W = 13312 > 12288
    _add(FB, 'nhwc4_cap', 1, 4, 1, 262144 + 37, cl=True)            # 4096 workgroups own 65 pixels each
    # --- channels-last, 8 channels a thread: bf16 x, not time-major
    for o in (False, True):
        _add(FB, 'nhwc8_%s' % dt(o), 4, 8, 5, 19, cl=True, x_bf16=True, o_bf16=o)       # P = 380: 2 PL = 512
        _add(ALL if o else FB, 'nhwc8_%s' % dt(o), 4, 128, 9, 57, cl=True, x_bf16=True, o_bf16=o)   # P = 2052: 3 trips
    _add(FB, 'nhwc8_4trips', 4, 256, 9, 57, cl=True, x_bf16=True, o_bf16=True)          # 129 chunks on 32 workgroups
    _add(FB, 'nhwc8', 3, 1024, 5, 11, cl=True, x_bf16=True)
    _add(FB, 'nhwc8_p1', 1, 8, 1, 1, cl=True, x_bf16=True)
    _add(FB, 'nhwc8_eval_bias', 4, 32, 5, 19, cl=True, x_bf16=True, o_bf16=True, training=False, bias=True)
    _add(FB, 'nhwc8_lohi', 4, 64, 5, 19, cl=True, x_bf16=True, lo=-1.5, hi=2.25)
    # --- LDS-transposing time-major: 8 rows a tile at C W = 352 (H = 3, B = 5: a tile spans three
    # utterances, 15 rows are no multiple of 8), 6 at 2048, 1 at 12288, the 2048-workgroup cap
    for xb in (False, True):
        for o in (False, True):
            _add(FB, 'tm_x%s_%s' % (_t(xb), dt(o)), 5, 32, 3, 11, cl=True, tm=True, x_bf16=xb, o_bf16=o)
    _add(ALL, 'tm_bias', 5, 32, 3, 11, cl=True, tm=True, bias=True)
    _add(FB, 'tm_6rows', 2, 128, 9, 16, cl=True, tm=True)
    _add(FB, 'tm_1row', 2, 1024, 3, 12, cl=True, tm=True)
    _add(FB, 'tm_cap_w1', 2341, 8, 7, 1, cl=True, tm=True)           # 16387 rows: 2049 tiles
    _add(FB, 'tm_h1', 11, 8, 1, 4, cl=True, tm=True, x_bf16=True)
    _add(FB, 'tm_eval_bias', 5, 32, 3, 11, cl=True, tm=True, x_bf16=True, training=False, bias=True)
    _add(FB, 'tm_lohi', 5, 32, 3, 11, cl=True, tm=True, lo=-1.5, hi=2.25)
    # --- |mean| / std = 64 in every channel, through the bias and in x itself: all statistics kernels
    for kind in ('offset_bias', 'offset_x'):
        b = kind == 'offset_bias'
        _add('fwd', kind + '_nchw', 3, 3, 9, 37, kind=kind, bias=b)
        _add('fwd', kind + '_nhwc4', 3, 32, 5, 11, cl=True, kind=kind, bias=b)
        _add('fwd', kind + '_nhwc4_c1024', 3, 1024, 5, 11, cl=True, kind=kind, bias=b)
        _add('fwd', kind + '_xbf16', 4, 32, 5, 19, cl=True, x_bf16=True, kind=kind, bias=b)
    # --- one NaN in x
    for tr in (False, True):
        t = 'nan_train' if tr else 'nan_eval'
        _add('fwd', t + '_nchw', 2, 3, 5, 7, kind='nan', training=tr)
        _add('fwd', t + '_nhwc4', 3, 16, 5, 11, cl=True, kind='nan', training=tr)
        _add('fwd', t + '_nhwc8', 4, 8, 5, 19, cl=True, x_bf16=True, o_bf16=True, kind='nan', training=tr)
        _add('fwd', t + '_tm', 5, 32, 3, 11, cl=True, tm=True, kind='nan', training=tr)
    _add('bwd', 'nan_train_nchw', 2, 3, 5, 7, kind='nan')
    _add('bwd', 'nan_train_nhwc4', 3, 16, 5, 11, cl=True, kind='nan')
    # --- exact integers, both clamp pairs, every family
    for lo, hi, t in ((0.0, 20.0, 'exact'), (-1.5, 2.25, 'exact_lohi')):
        kw = dict(kind='exact', training=False, bias=True, lo=lo, hi=hi)
        _add(FB, t + '_nchw', 3, 3, 9, 37, **kw)
        _add(FB, t + '_nchw_tm_obf16', 3, 3, 9, 37, tm=True, o_bf16=True, **kw)
        _add(FB, t + '_nhwc4', 3, 64, 5, 11, cl=True, **kw)
        _add(FB, t + '_nhwc4_c1024', 3, 1024, 5, 11, cl=True, **kw)
        _add(FB, t + '_nhwc4_tm', 3, 4, 7, 5, cl=True, tm=True, x_bf16=True, o_bf16=True, **kw)
        _add(FB, t + '_nhwc8', 4, 128, 9, 57, cl=True, x_bf16=True, o_bf16=True, **kw)
        _add(FB, t + '_tm', 5, 32, 3, 11, cl=True, tm=True, **kw)
        _add(FB, t + '_tm_6rows', 2, 128, 9, 16, cl=True, tm=True, x_bf16=True, o_bf16=True, **kw)


_matrix()


def cases():
    return list(SPECS)


def exact_cases():
    return [n for n, s in SPECS.items() if s['kind'] == 'exact']


# ------------------------------------------------------------------ inputs

def _bf(a):
    return bf16_f32(bf16_rne(np.asarray(a, F32))).reshape(np.shape(a))


def exact_case(spec, rng):
    """the exact-integer form: every product and every partial sum is exact in fp32 in any order"""
    B, C, H, W = (spec[k] for k in 'BCHW')
    lo, hi = spec['lo'], spec['hi']
    step = 1.0 if lo == 0.0 else 0.25             # y is a multiple of `step`; lo and hi are too
    inp = dict(running_var=rng.choice([0.25, 1.0, 4.0], C).astype(F32),
               running_mean=rng.integers(-3, 4, C).astype(F32),
               conv_bias=rng.integers(-3, 4, C).astype(F32),
               beta=(rng.integers(0, 9, C) * step * 2).astype(F32), eps=0.0)
    invstd = 1.0 / np.sqrt(inp['running_var'].astype(F64))
    # gamma * invstd in {step, 2 step}, either sign: gamma is a power of two
    inp['gamma'] = (rng.choice([step, 2 * step], C) * rng.choice([1.0, 1.0, -1.0], C) / invstd).astype(F32)
    inp['x'] = rng.integers(-12, 13, (B, C, H, W)).astype(F32)
    inp['dy'] = rng.integers(-4, 5, (B, C, H, W)).astype(F32)
    return inp


def build(name):
    """the inputs of a case, seeded by its shape and data kind (not by its op: fwd and bwd share them)"""
    spec = SPECS[name]
    B, C, H, W = (spec[k] for k in 'BCHW')
    seed = zlib.crc32(('%s %d %d %d %d %s' % (spec['kind'], B, C, H, W, spec['lo'])).encode())
    rng = np.random.default_rng(seed)
    lo, hi = spec['lo'], spec['hi']
    span = hi - lo
    if spec['kind'] == 'exact':
        inp = exact_case(spec, rng)
    else:
        inp = dict(eps=EPS)
        inp['gamma'] = (span * (0.025 + 0.4 * rng.random(C)) * rng.choice([1.0, 1.0, 1.0, -1.0], C)).astype(F32)
        inp['beta'] = (lo + span * (0.3 + 0.2 * rng.standard_normal(C))).astype(F32)
        inp['running_mean'] = (0.3 * rng.standard_normal(C)).astype(F32)
        inp['running_var'] = (rng.random(C) + 0.5).astype(F32)
        x = 1.5 * rng.standard_normal((B, C, H, W)) + 0.2
        inp['conv_bias'] = rng.standard_normal(C).astype(F32)
        off = 64 * 1.5 * rng.choice([1.0, -1.0], C)
        if spec['kind'] == 'offset_bias':
            inp['conv_bias'] = off.astype(F32)
            x -= 0.2
        elif spec['kind'] == 'offset_x':
            x += off[None, :, None, None] - 0.2
        inp['x'] = x.astype(F32)
        inp['dy'] = rng.standard_normal((B, C, H, W)).astype(F32)
        if spec['kind'] == 'nan':
            inp['nan_at'] = (B - 1, C // 2, H // 2, W - 1)
            inp['x'][inp['nan_at']] = NAN
    if spec['x_bf16']:
        inp['x'] = _bf(inp['x'])
    if spec['o_bf16']:
        inp['dy'] = _bf(inp['dy'])
    if not spec['bias']:
        inp['conv_bias'] = None
    inp.update(spec=spec, momentum=MOMENTUM, n=float(B * H * W))
    if spec['op'] == 'fwd':
        del inp['dy']
        if spec['chan_sums']:
            x = inp['x'].astype(F64)
            inp['chan_sums'] = np.stack([x.sum((0, 2, 3)), (x * x).sum((0, 2, 3))])
        if spec['null_running']:
            inp['running_mean'] = inp['running_var'] = None
        return inp
    # the backward launches read the statistics a forward saved: the fp64 ones, rounded to fp32
    st = _ref_stats(dict(inp, spec=dict(spec, chan_sums=False)))
    with np.errstate(invalid='ignore'):
        inp['save_mean'], inp['save_invstd'] = st['mean'].astype(F32), st['invstd'].astype(F32)
    if spec['op'] == 'bwd_phase2':        # the sums of two replicas that saw the same data
        w = _ref_bwd(dict(inp, spec=dict(spec, op='bwd_phase1')))
        inp['sums'] = 2.0 * w['sums']
        inp['n_total'] = 2.0 * inp['n']
    return inp


# ------------------------------------------------------------------ fp64 references

def _c(a):
    return np.asarray(a, F64)[None, :, None, None]


def _bias(inp):
    C = inp['spec']['C']
    return np.zeros(C) if inp['conv_bias'] is None else inp['conv_bias'].astype(F64)


def hardtanh(y, lo, hi):
    with np.errstate(invalid='ignore'):
        return np.where(y < lo, lo, np.where(y > hi, hi, y))


def passes(y, lo, hi):
    """torch's hardtanh_backward: the gradient passes where lo < y < hi strictly (not at a NaN)"""
    with np.errstate(invalid='ignore'):
        return (y > lo) & (y < hi)


def _ref_stats(inp):
    spec = inp['spec']
    n, eps = inp['n'], F64(F32(inp['eps']))
    bias = _bias(inp)
    if not spec['training']:
        mean, var = inp['running_mean'].astype(F64), None
        invstd = 1.0 / np.sqrt(inp['running_var'].astype(F64) + eps)
    elif spec['chan_sums']:
        mx = inp['chan_sums'][0] / n
        var = np.maximum(inp['chan_sums'][1] / n - mx * mx, 0.0)
        mean = mx + bias
        invstd = 1.0 / np.sqrt(var + eps)
    else:
        v = inp['x'].astype(F64) + _c(bias)
        mean = v.mean((0, 2, 3))
        var = ((v - _c(mean)) ** 2).mean((0, 2, 3))
        invstd = 1.0 / np.sqrt(var + eps)
    return dict(mean=mean, var=var, invstd=invstd)


def _ref_fwd(inp):
    spec = inp['spec']
    st = _ref_stats(inp)
    mean, invstd, n = st['mean'], st['invstd'], inp['n']
    v = inp['x'].astype(F64) + _c(_bias(inp))
    y = (v - _c(mean)) * _c(invstd) * _c(inp['gamma']) + _c(inp['beta'])
    want = dict(y=y, out=hardtanh(y, spec['lo'], spec['hi']), save_mean=mean, save_invstd=invstd, var=st['var'],
                running_mean=None, running_var=None)
    if inp['running_mean'] is not None:
        rm, rv = inp['running_mean'].astype(F64), inp['running_var'].astype(F64)
        if spec['training']:
            mom = F64(F32(inp['momentum']))
            unbiased = st['var'] * n / (n - 1.0) if n > 1 else st['var']
            rm, rv = (1.0 - mom) * rm + mom * mean, (1.0 - mom) * rv + mom * unbiased
        want.update(running_mean=rm, running_var=rv)
    return want


def _ref_bwd(inp, mean=None, invstd=None):
    """from the case's fp32 save_mean / save_invstd (or, for the comparison with torch, unrounded ones)"""
    spec = inp['spec']
    op, lo, hi = spec['op'], spec['lo'], spec['hi']
    mean = inp['save_mean'].astype(F64) if mean is None else mean
    invstd = inp['save_invstd'].astype(F64) if invstd is None else invstd
    g, be, bias = inp['gamma'].astype(F64), inp['beta'].astype(F64), _bias(inp)
    xh = (inp['x'].astype(F64) + _c(bias) - _c(mean)) * _c(invstd)
    y = xh * _c(g) + _c(be)
    mask = passes(y, lo, hi)
    d = np.where(mask, inp['dy'].astype(F64), 0.0)
    want = dict(y=y, xh=xh, d=d, dx=None, dgamma=None, dbeta=None, dconv_bias=None, sums=None)
    if op == 'bwd_phase2':
        s1, s2, n = inp['sums'][0::2], inp['sums'][1::2], inp['n_total']
        want['sums'] = inp['sums']
    else:
        s1, s2, n = d.sum((0, 2, 3)), (d * xh).sum((0, 2, 3)), inp['n']
        want['sums'] = np.stack([s1, s2], 1).reshape(-1)
        want.update(dbeta=s1, dgamma=s2)
        if inp['conv_bias'] is not None:
            want['dconv_bias'] = np.zeros_like(s1) if spec['training'] else g * invstd * s1
    if op != 'bwd_phase1':
        k1, k2 = (s1 / n, s2 / n) if spec['training'] else (np.zeros_like(s1), np.zeros_like(s1))
        want['dx'] = _c(g * invstd) * (d - _c(k1) - xh * _c(k2))
        want['k'] = (k1, k2)
    return want


def reference(op, inp):
    assert op == inp['spec']['op']
    return _ref_fwd(inp) if op == 'fwd' else _ref_bwd(inp)


# ------------------------------------------------------------------ tolerances

def _chan_sum(a):
    return a.sum((0, 2, 3))


def _tol_fwd(inp, want):
    spec = inp['spec']
    g, be, bias = inp['gamma'].astype(F64), inp['beta'].astype(F64), _bias(inp)
    mean, invstd, n = want['save_mean'], want['save_invstd'], inp['n']
    x = inp['x'].astype(F64)
    dev = np.abs(x + _c(bias) - _c(mean))
    tol = {}
    if not spec['training']:
        dmean, dis, dvar = np.zeros_like(mean), 3 * U * invstd, None
    else:
        if spec['chan_sums']:
            dsum, dvar = 0.0, 8 * 2.0 ** -52 * inp['chan_sums'][1] / n
        else:
            D = depth(stats_path(spec), spec)
            mad, maxdev = dev.mean((0, 2, 3)), dev.max((0, 2, 3))
            dsum = (D + 1) * U * (mad + maxdev)
            dvar = (D + 3) * U * (want['var'] + maxdev ** 2)
        dmean = dsum + U * np.abs(mean)
        dis = 0.5 * invstd ** 3 * dvar + U * invstd
    tol['save_mean'], tol['save_invstd'] = dmean, dis
    sc, mp = g * invstd, mean - bias
    sh = be - mp * sc
    tol['out'] = (np.abs(_c(g)) * dev * _c(dis) + _c(np.abs(sc) * dmean)
                  + U * (np.abs(x * _c(sc)) + _c(2 * np.abs(mp * sc) + np.abs(sh)) + np.abs(want['y'])))
    if want['running_mean'] is not None:
        rm, rv = inp['running_mean'].astype(F64), inp['running_var'].astype(F64)
        if spec['training']:
            mom = F64(F32(inp['momentum']))
            scale = n / (n - 1.0) if n > 1 else 1.0
            tol['running_mean'] = mom * dmean + 3 * U * (np.abs((1 - mom) * rm) + np.abs(mom * mean) + np.abs(want['running_mean']))
            tol['running_var'] = mom * scale * dvar + 3 * U * ((1 - mom) * rv + mom * scale * want['var'] + want['running_var'])
        else:
            tol['running_mean'], tol['running_var'] = np.zeros_like(rm), np.zeros_like(rv)
    return tol


def _tol_bwd(inp, want):
    spec = inp['spec']
    op, lo, hi = spec['op'], spec['lo'], spec['hi']
    g, bias = inp['gamma'].astype(F64), _bias(inp)
    mean, invstd = inp['save_mean'].astype(F64), inp['save_invstd'].astype(F64)
    xh, y, d, dy = want['xh'], want['y'], want['d'], inp['dy'].astype(F64)
    exh = U * (_c(np.abs(mean - bias) * invstd) + 2 * np.abs(xh))
    ey = _c(np.abs(g)) * exh + U * np.abs(y)
    with np.errstate(invalid='ignore'):
        amb = (np.abs(y - lo) <= ey) | (np.abs(y - hi) <= ey)
    tol = dict(ambiguous=amb)
    D = depth(apply_path(spec), spec)
    a1, a2 = np.abs(np.where(amb, 0.0, d)), np.abs(np.where(amb, 0.0, d * xh))
    w1, w2 = np.where(amb, np.abs(dy), 0.0), np.where(amb, np.abs(dy * xh), 0.0)
    if op == 'bwd_phase2':
        ds1 = ds2 = np.zeros_like(mean)
        s1, s2, n = inp['sums'][0::2], inp['sums'][1::2], inp['n_total']
    else:
        ds1 = D * U * _chan_sum(a1) + _chan_sum(w1)
        ds2 = (D + 1) * U * _chan_sum(a2) + _chan_sum(a1 * exh) + _chan_sum(w2)
        s1, s2, n = want['dbeta'], want['dgamma'], inp['n']
        tol['sums'] = np.stack([ds1, ds2], 1).reshape(-1)
        tol['dbeta'], tol['dgamma'] = ds1 + U * np.abs(s1), ds2 + U * np.abs(s2)
        if want['dconv_bias'] is not None:
            tol['dconv_bias'] = np.abs(g * invstd) * (ds1 + U * np.abs(s1)) + 3 * U * np.abs(want['dconv_bias'])
    if op != 'bwd_phase1':
        k1, k2 = want['k']
        if spec['training']:
            dk1, dk2 = ds1 / n + U * np.abs(k1), ds2 / n + U * np.abs(k2)
            inner = d - _c(k1) - xh * _c(k2)
            e_in = (_c(dk1) + np.abs(xh) * _c(dk2) + exh * _c(np.abs(k2))
                    + U * (np.abs(xh * _c(k2)) + np.abs(d - _c(k1)) + np.abs(inner)))
        else:
            e_in = 0.0
        tol['dx'] = _c(np.abs(g * invstd)) * e_in + 2 * U * np.abs(want['dx'])
    return tol


def tolerances(op, inp, want):
    """per output the absolute tolerance (module docstring); `ambiguous`: the elements left out"""
    with np.errstate(invalid='ignore', over='ignore'):
        return _tol_fwd(inp, want) if op == 'fwd' else _tol_bwd(inp, want)


def left_out_cap(spec):
    return -(-spec['B'] * spec['C'] * spec['H'] * spec['W'] // CAP)


# ------------------------------------------------------------------ the judge

def _interval(name, got, lo_v, hi_v, want, bf16, skip, bad, stats, tol):
    """got within [lo_v, hi_v] (their bf16 roundings for a bf16 output), NaN exactly where want is"""
    got = np.asarray(got, F64)
    wn = np.isnan(want)
    if not np.array_equal(np.isnan(got), wn):
        bad.append('%s: NaN at %d entries, the reference at %d' % (name, np.isnan(got).sum(), wn.sum()))
        return
    if bf16:
        with np.errstate(invalid='ignore', over='ignore'):
            lo_v = bf16_f32(bf16_rne(lo_v.astype(F32))).reshape(got.shape).astype(F64)
            hi_v = bf16_f32(bf16_rne(hi_v.astype(F32))).reshape(got.shape).astype(F64)
            tol = np.maximum(tol, np.maximum(want - lo_v, hi_v - want))      # (for the share only)
    with np.errstate(invalid='ignore'):
        out = ~wn & ~skip & ((got < lo_v) | (got > hi_v))
        err = np.where(wn | skip, 0.0, np.abs(got - want))
    stats[name] = float(err.max(initial=0.0))
    with np.errstate(invalid='ignore', divide='ignore'):
        stats[name + ':share'] = float(np.nan_to_num(np.where(wn | skip | (tol <= 0), 0.0, err / tol)).max(initial=0.0))
    if out.any():
        i = np.unravel_index(np.argmax(np.where(out, np.maximum(got - hi_v, lo_v - got), -1.0)), got.shape)
        bad.append('%s: %d entries outside, worst at %s: got %.9g, want %.9g in [%.9g, %.9g]' % (
            name, out.sum(), i, got[i], want[i], lo_v[i], hi_v[i]))


def _vector(name, got, want, tol, bad, stats):
    if want is None:
        return
    if got is None:
        bad.append('%s: missing' % name)
        return
    z = np.zeros(np.shape(want), bool)
    _interval(name, got, want - tol, want + tol, want, False, z, bad, stats, tol)


def _untouched(name, got, bad):
    if got is not None and not (np.asarray(got) == POISON).all():
        bad.append('%s: %d entries written by a launch that must leave it alone' % (
            name, (np.asarray(got) != POISON).sum()))


def judge(op, inp, got, want, tol, stats=None):
    """the complaints about the outputs `got` of one launch (logical arrays; a bf16 output as the
    fp32 values of its halves; an output the launch was not given: None).  tol None: equality."""
    spec = inp['spec']
    bad, stats = [], ({} if stats is None else stats)
    if tol is None:                                         # the exact cases
        for k in (('out', 'save_mean', 'save_invstd', 'running_mean', 'running_var') if op == 'fwd'
                  else ('dx', 'dgamma', 'dbeta', 'dconv_bias')):
            if want[k] is not None and not np.array_equal(np.asarray(got[k], F64), want[k]):
                bad.append('%s: %d entries differ' % (k, (np.asarray(got[k], F64) != want[k]).sum()))
        return bad
    if op == 'fwd':
        t = tol['out']
        none = np.zeros(t.shape, bool)
        _interval('out', got['out'], hardtanh(want['y'] - t, spec['lo'], spec['hi']),
                  hardtanh(want['y'] + t, spec['lo'], spec['hi']), want['out'], spec['o_bf16'], none, bad, stats, t)
        for k in ('save_mean', 'save_invstd', 'running_mean', 'running_var'):
            _vector(k, got[k], want[k], tol.get(k), bad, stats)
        return bad
    amb = tol['ambiguous']
    if amb.sum() > left_out_cap(spec):
        bad.append('%d elements within their tolerance of a clamp, the cap is %d' % (amb.sum(), left_out_cap(spec)))
    if op == 'bwd_phase1':
        _untouched('dx', got['dx'], bad)
    else:
        _interval('dx', got['dx'], want['dx'] - tol['dx'], want['dx'] + tol['dx'], want['dx'],
                  spec['x_bf16'], amb, bad, stats, tol['dx'])
    if op == 'bwd_phase2':
        for k in ('dgamma', 'dbeta', 'dconv_bias'):
            _untouched(k, got[k], bad)
        if not np.array_equal(got['sums'], want['sums']):
            bad.append('sums: phase 2 changed the sums it was given')
    else:
        for k in ('dgamma', 'dbeta', 'dconv_bias'):
            _vector(k, got[k], want[k], tol.get(k), bad, stats)
        if op == 'bwd_phase1':
            _vector('sums', got['sums'], want['sums'], tol['sums'], bad, stats)
    return bad


# ------------------------------------------------------------------ the kernels' arithmetic in fp32

def _fma(a, b, c):
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _pad(a, axis, size):
    w = [(0, 0)] * a.ndim
    w[axis] = (0, size - a.shape[axis])
    return np.pad(a, w)


def _serial(T, axis):
    """fp32 adds along `axis`, in order, from 0"""
    T = np.moveaxis(T, axis, 0)
    acc = np.zeros(T.shape[1:], F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(T.shape[0]):
            acc = acc + T[k]
    return acc


def _ksum(path, terms, spec, mut=None):
    """per-channel sums [C] (double) of fp32 terms [B, C, H, W] in the order of the kernels of `path`"""
    B, C, H, W = terms.shape
    P = B * H * W
    terms = np.asarray(terms, F32)
    if path == 'nchw':
        T = _pad(terms.transpose(1, 0, 2, 3).reshape(C, B, H * W), 2, -(-H * W // 256) * 256)
        v = _serial(T.reshape(C, B, -1, 256), 2).reshape(C, B, 4, 64)
        with np.errstate(invalid='ignore'):
            for o in (32, 16, 8, 4, 2, 1):
                v = v + v[..., np.arange(64) ^ o]
        tot = _serial(v[..., 0], 2)
    else:
        tc = terms.transpose(1, 0, 2, 3).reshape(C, P)
        if path == 'nhwc4':
            PL, G = 1024 // C, nwg(P)
            per = -(-P // G)
            T = _pad(tc, 1, G * per).reshape(C, G, per).copy()
            if mut == 'slice_last_pixel_dropped':
                for w in range(G):
                    last = min((w + 1) * per, P) - 1 - w * per
                    if last >= 0:
                        T[:, w, last] = 0
            K = -(-per // PL)
            T = _pad(T, 2, K * PL).reshape(C, G, K, PL)
        elif path == 'nhwc8':
            PL, G = 2048 // C, nwg(P)
            trips = -(-P // (2 * PL * G))
            T = _pad(tc, 1, trips * G * 2 * PL).reshape(C, trips, G, 2, PL).copy()
            if mut == 'second_trip_dropped':
                T[:, 1:] = 0
            T = T.transpose(0, 2, 1, 3, 4).reshape(C, G, trips * 2, PL)
        else:
            R, PL = tm_rows(C * W), 1024 // C
            tiles = -(-B * H // R)
            G = min(tiles, 2048)
            trips, K = -(-tiles // G), -(-R * W // PL)
            T = _pad(tc, 1, trips * G * R * W).reshape(C, trips, G, R * W).copy()
            if mut == 'second_trip_dropped':
                T[:, 1:] = 0
            T = _pad(T, 3, K * PL).reshape(C, trips, G, K, PL).transpose(0, 2, 1, 3, 4).reshape(C, G, trips * K, PL)
        tot = _serial(_serial(T, 2), 2)
    s = tot.astype(F64).sum(1)
    if mut == 'channels_ge_256_missing' and path != 'nchw':
        s[256:] = 0.0
    return s


def _round_out(v, bf16, mut):
    if not bf16:
        return v
    return bf16_f32((bf16_trunc if mut == 'bf16_truncates' else bf16_rne)(v)).reshape(v.shape)


def _c32(a):
    return np.asarray(a, F32)[None, :, None, None]


def _model_fwd(inp, mut):
    spec = inp['spec']
    B, C, H, W = (spec[k] for k in 'BCHW')
    x, n = inp['x'], inp['n']
    g, be = inp['gamma'], inp['beta']
    bias = inp['conv_bias']
    out = dict(running_mean=None if inp['running_mean'] is None else inp['running_mean'].copy(),
               running_var=None if inp['running_var'] is None else inp['running_var'].copy())
    with np.errstate(invalid='ignore', over='ignore'):
        if spec['training']:
            b64 = _bias(inp) if mut != 'bias_missing_from_mean' else 0.0
            if spec['chan_sums']:
                md = inp['chan_sums'][0] / n
                var = inp['chan_sums'][1] / n - md * md
                m = md + b64
            else:
                pv = x[0, :, 0, 0]
                d = x - _c32(pv)
                path = stats_path(spec)
                md = _ksum(path, d, spec, mut) / n
                var = _ksum(path, d * d, spec, mut) / n - md * md
                m = pv.astype(F64) + md + b64
            var = np.where(var < 0, 0.0, var)
            mean = m.astype(F32)
            invstd = (1.0 / np.sqrt(var + F64(F32(inp['eps'])))).astype(F32)
            if out['running_mean'] is not None:
                mom = F32(inp['momentum'])
                unb = var * n / (n - 1.0) if n > 1 and mut != 'biased_running_var' else var
                out['running_mean'] = (F32(1) - mom) * out['running_mean'] + mom * mean
                out['running_var'] = (F32(1) - mom) * out['running_var'] + mom * unb.astype(F32)
        else:
            mean = inp['running_mean'].copy()
            invstd = F32(1) / np.sqrt(inp['running_var'] + F32(inp['eps']))
        sc = g * invstd
        sh = be - (mean - (bias if bias is not None else F32(0))) * sc
        y = _fma(x, _c32(sc), _c32(sh))
        lo, hi = F32(spec['lo']), F32(spec['hi'])
        y = np.fmin(np.fmax(y, lo), hi) if mut == 'nan_clamped_to_lo' else hardtanh(y, lo, hi).astype(F32)
    y = _round_out(y, spec['o_bf16'], mut)
    if mut == 'tm_index_b_h_swapped' and spec['tm']:
        y = from_storage(np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(-1), (B, C, H, W), 'tm')
    out.update(out=y, save_mean=mean, save_invstd=invstd)
    return out


def _model_bwd(inp, mut):
    spec = inp['spec']
    op, lo, hi = spec['op'], F32(spec['lo']), F32(spec['hi'])
    B, C, H, W = (spec[k] for k in 'BCHW')
    x, dy, g, be = inp['x'], inp['dy'], inp['gamma'], inp['beta']
    mean, invstd, bias = inp['save_mean'], inp['save_invstd'], inp['conv_bias']
    path = apply_path(spec)
    if mut == 'tm_index_b_h_swapped' and spec['tm']:
        dy = np.ascontiguousarray(to_storage(dy, 'tm').reshape(B, H, C, W).transpose(0, 2, 1, 3))
    if mut == 'tile_row_from_wrong_batch' and path == 'tm':
        R = tm_rows(C * W)
        dy = dy.copy()
        for r in range(B * H):
            b, h, b0 = r // H, r % H, (r // R * R) // H
            dy[b, :, h] = inp['dy'][b0, :, h]
    out = dict(dx=np.full(x.shape, POISON, F32), sums=None)
    for k in ('dgamma', 'dbeta', 'dconv_bias'):
        out[k] = None if (k == 'dconv_bias' and bias is None) else np.full(C, POISON, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        m = mean - (bias if bias is not None else F32(0))
        xh = (x - _c32(m)) * _c32(invstd)
        y = _fma(xh, _c32(g), _c32(be))
        above_lo = (y >= lo) if mut == 'mask_ge_lo' else (y > lo)
        below_hi = (y <= hi) if mut == 'mask_le_hi' else (y < hi)
        d = np.where(above_lo & below_hi, dy, F32(0))
        if op == 'bwd_phase2':
            sums, n = inp['sums'], inp['n_total']
        else:
            sums = np.stack([_ksum(path, d, spec, mut), _ksum(path, d * xh, spec, mut)], 1).reshape(-1)
            n = inp['n']
            out['dbeta'], out['dgamma'] = sums[0::2].astype(F32), sums[1::2].astype(F32)
            if bias is not None:
                out['dconv_bias'] = np.zeros(C, F32) if spec['training'] else g * invstd * sums[0::2].astype(F32)
        out['sums'] = sums
        if op != 'bwd_phase1':
            k1 = (sums[0::2] / n).astype(F32) if spec['training'] else np.zeros(C, F32)
            k2 = (sums[1::2] / n).astype(F32) if spec['training'] and mut != 'k2_dropped' else np.zeros(C, F32)
            dx = _c32(g * invstd) * _fma(-xh, _c32(k2), d - _c32(k1))
            out['dx'] = _round_out(dx, spec['x_bf16'], mut)
    return out


def model(op, inp, mut=None):
    """what the kernels compute, in numpy fp32 in their order; `mut`: one of MUTANTS"""
    assert mut is None or mut in MUTANTS
    return _model_fwd(inp, mut) if op == 'fwd' else _model_bwd(inp, mut)
