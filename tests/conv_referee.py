"""Referee of the convolution kernels of csrc/conv.hip, one launch at a time: forward, input
gradient and weight gradient of the 32 -> 32 channel 7x7 convolution (asr_conv7x7c32_*), forward
and weight gradient of the first convolution on one and on three input channels
(asr_conv1_7x7s2_*, asr_conv1c_7x7s2_*).

Written from the contract in include/asr_amd.h and the layout comments of csrc/conv.hip; numpy and
torch on the CPU, no native calls.  All tensors here are in LOGICAL layout ([B, C, H, W]; the
kernels' memory is channels-last, the caller permutes).  Parts:

* `plan(op, shape)`: the launchers' host arithmetic (rows per workgroup, LDS pitch and size,
  template classes), ported to Python: None for a shape the launcher answers with
  ASR_EUNSUPPORTED.  `cases()` takes its boundaries from it, the gate sweep of
  tests/test_conv_referee.py holds it against the library's own queries.
* `cases()`: one entry per (op, shape), the smallest shapes that reach each code path.
* `integer_inputs(case)` / `gaussian_inputs(case)`: the operands.  The integer ones are small
  integers, exact in bf16, sparse enough that every output of the fp64 reference is an integer the
  output type holds exactly (|y|, |dx| <= 128; |dw| < 2^24): whatever order a kernel sums in, it
  must produce those very values, and one mis-indexed element is an exact mismatch.
* `reference(case, inp)`: torch's conv2d / conv2d_input / conv2d_weight in float64 on the operands
  rounded the way the kernels round them (bf16, round to nearest even); `S`, the same convolution
  of the absolute values; `rms32`, the RMS rounding error of bf16_rne(fp32 CPU convolution).
* `judge(case, got, want, kind)`: the complaints about one launch's outputs.
  - kind 'integer': every element equal; the channel sums equal to the reference's whenever
    sum(y^2) < 2^24 (every fp32 partial sum is then an exactly represented integer), else within
    1e-5 of the sums of the kernel's own outputs.
  - kind 'gaussian', three rules, none of them tuned on a kernel:
    1. per element |got - want| <= r(want) + K 2^-23 S, with r = half a bf16 ulp of want (bf16
       outputs) or 2^-23 |want| (fp32 outputs) and K the number of products in the sum.  This
       grants one FULL fp32 ulp of the running sum's bound per addition, not half: the
       architecture guides do not promise round-to-nearest inside an MFMA accumulation.  Per
       element: an edge pixel with a small S gets a small allowance, an element no window covers
       (S = 0) none.
    2. bf16 outputs: the mean of sign(want) (got - want) / ulp_bf16(want) within +-0.02
       (round-to-nearest gives 0 with a standard error below 0.003 at the >= 10^4 elements every
       such case has, truncation -0.5).
    3. bf16 outputs: the RMS of (got - want) / ulp_bf16(want) at most 5 % above the same
       statistic of bf16_rne(fp32 CPU convolution of the same operands) (near 1 / sqrt(12);
       sampling noise below 1 % at 10^4 elements).
* `model(case, inp, mut)`: the reference arithmetic in fp32 with one wrong term `mut` (None: the
  unmutated model), for the CPU proof in tests/test_conv_referee.py that the model passes every
  judge and every mutant is rejected."""
import numpy as np
import torch
import torch.nn.functional as F

POISON_H = 0x5ead                   # pre-fill of bf16 outputs (as bits): 6.2e18, never an answer
POISON_F = -777.25                  # of fp32 outputs
OPS = ('c32_fwd', 'c32_dgrad', 'c32_wgrad', 'c1_fwd', 'c1_wgrad', 'c1c_fwd', 'c1c_wgrad')
BF16_OUT = ('c32_fwd', 'c32_dgrad', 'c1_fwd', 'c1c_fwd')
FWD = ('c32_fwd', 'c1_fwd', 'c1c_fwd')
MUTANTS = ('tap66_dropped', 'last_column_unwritten', 'partial_block_last_row_unwritten',
           'ci_30_31_swapped', 'dgrad_class2_dropped', 'dx_trailing_rows_unwritten',
           'bf16_truncated', 'acc_bf16_every_16', 'sums_miss_last_group', 'wgrad_misses_last_chunk')

# ---- constants of csrc/conv.hip ------------------------------------------------------------
KS, CH, PIX = 7, 32, 80
FWD_PIX, FWD_MAXQ = 128, 15         # pixels per forward workgroup; DMA slots per wave
DG_PIX, DG_NT = 192, 6              # pixels per input-gradient workgroup and class
WGRAD_WGS, WGRAD_NT, NX_MAX, ND_MAX = 256, 448, 8, 3
C1_ROWS, C1_WGS = 16, 1024          # conv1: output rows per chunk, persistent workgroups
C1C_ROWS, C1C_FWD_WGS = 8, 768      # three channels: rows per chunk, forward workgroups
SUMS_WGS = 1 << 17                  # forward workgroups whose channel sums fit the workspace


def _pick_row_pitch(min_pitch, per_row, step, npix, ntiles):
    """pick_row_pitch: the pitch in [min_pitch, min_pitch + 256] with the fewest ds_read_b128 bank
    conflicts over the first tiles (first minimum wins)"""
    grp = ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27),
           (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31))
    best, best_cost = min_pitch, 1 << 30
    for P in range(min_pitch, min_pitch + 257, 16):
        cost = 0
        for tile in range(ntiles):
            for g in grp:
                addr, cnt, worst = {}, {}, 1
                for i in g:
                    m = min(32 * tile + i, npix - 1)
                    r = m // per_row
                    a = r * step * P + (m - r * per_row) * PIX
                    for k in range(4):
                        b = (a // 4 + k) & 63
                        if addr.get(b) != a + 4 * k:
                            addr[b] = a + 4 * k
                            cnt[b] = cnt.get(b, 0) + 1
                            worst = max(worst, cnt[b])
                cost += worst
        if cost < best_cost:
            best_cost, best = cost, P
    return best


_PLANS = {}


def plan(op, shape):
    """the launcher's geometry for `shape` ((B, H, W, stride_h) for c32_*, (B, T, F) for c1*), or
    None where it answers ASR_EUNSUPPORTED.  Forward plans are those of a call WITH chan_sums."""
    key = (op,) + tuple(shape)
    if key not in _PLANS:
        _PLANS[key] = _plan(op, shape)
    return _PLANS[key]


def _plan(op, shape):
    if op.startswith('c32'):
        B, H, W, sh = shape
        assert B > 0 and H >= KS and W >= KS
        Ho, Wo = (H - KS) // sh + 1, W - KS + 1
        if op == 'c32_fwd':
            if sh not in (1, 3) or Wo > 48:
                return None
            R = min(16, FWD_PIX // Wo)
            pitch = _pick_row_pitch(W * PIX, Wo, sh, R * Wo, 4)
            img = -(-((sh * (R - 1) + KS) * pitch) // 1024) * 1024
            lds = img + img // 8 + 4 * 4096 + 2048
            if H * W * 64 >= 2 ** 31 or img > 4 * FWD_MAXQ * 1024 or lds > 80 * 1024:
                return None
            return dict(Ho=Ho, Wo=Wo, R=R, pitch=pitch, lds=lds, items=B * -(-Ho // R))
        if sh != 3:
            return None
        if op == 'c32_dgrad':
            if W > 48:
                return None
            Rq = min(16, DG_PIX // W)
            pitch = _pick_row_pitch((Wo + 12) * PIX, W, 1, Rq * W, DG_NT)
            img = -(-((Rq + 2) * pitch) // 1024) * 1024
            lds = img + DG_NT * 4 * 64 * 16 + 2 * DG_PIX * CH * 2
            if B * Ho * Wo * 64 >= 2 ** 31 or lds > 80 * 1024 or img > 28 * 1024:
                return None
            nq = (H + 2) // 3
            return dict(Ho=Ho, Wo=Wo, Rq=Rq, nq=nq, pitch=pitch, lds=lds, items=B * -(-nq // Rq))
        if Wo > 48:
            return None
        KW, rows = -(-Wo // 16), 8
        while rows >= 1:
            xrows = 3 * (rows - 1) + KS
            lds = (xrows * W + 24) * PIX + rows * 16 * KW * PIX
            if lds <= 72 * 1024 and xrows * W * 4 <= NX_MAX * WGRAD_NT and rows * 16 * KW * 4 <= ND_MAX * WGRAD_NT:
                break
            rows >>= 1
        if rows < 1:
            return None
        return dict(Ho=Ho, Wo=Wo, KW=KW, rows=rows, lds=lds, items=B * -(-Ho // rows))
    B, T, Fw = shape
    assert B > 0 and T > 0 and Fw >= KS
    To, Fo = T + 6, (Fw - KS) // 2 + 1
    if Fo > 64:
        return None
    if op in ('c1_fwd', 'c1_wgrad'):
        items = B * -(-To // C1_ROWS)
        if op == 'c1_fwd':
            ntiles = -(-C1_ROWS * Fo // 32)
            lds = (C1_ROWS + 8) * Fo * 16 + ntiles * 32 * CH * 2 + 512 * 4
            if items > SUMS_WGS or lds > 64 * 1024:
                return None
            return dict(To=To, Fo=Fo, rows=C1_ROWS, lds=lds, items=items)
        lds = max((C1_ROWS + 8) * Fo * 16 + C1_ROWS * Fo * PIX, 4 * 2 * 1024 * 4)
        if lds > 64 * 1024:
            return None
        di, wpt = -(-C1_ROWS * Fo * 4 // 256), -(-(C1_ROWS + 8) * Fo // 256)
        cls = (5, 2) if di <= 5 and wpt <= 2 else ((8, 3) if di <= 8 and wpt <= 3 else (16, 6))
        return dict(To=To, Fo=Fo, rows=C1_ROWS, lds=lds, cls=cls, items=items)
    if Fo & 1:
        return None
    R = C1C_ROWS
    items = B * -(-To // R)
    FP = (2 * (Fo - 1) + 8 + 3) & ~3
    rpt = -(-(R + 8) * Fw * 3 // 256)
    if op == 'c1c_fwd':
        ntiles = -(-R * Fo // 32)
        otail = max(ntiles * 32 * CH * 2 + 512 * 4, 3 * (R + 8) * FP * 2)
        lds = 3 * (R + 8) * Fo * 16 + otail
        if T * Fw * 3 * 4 * B >= 2 ** 40 or items > SUMS_WGS or lds > 64 * 1024 or rpt > 24:
            return None
        return dict(To=To, Fo=Fo, rows=R, lds=lds, rpt=16 if rpt <= 16 else 24, items=items)
    lds = max(3 * (R + 8) * Fo * 16 + R * Fo * PIX + 3 * (R + 8) * FP * 2, 4 * 1024 * 4)
    di = -(-R * Fo * 4 // 256)
    if lds > 64 * 1024 or di > 8 or rpt > 24:
        return None
    return dict(To=To, Fo=Fo, rows=R, lds=lds, cls=(5, 16) if di <= 5 and rpt <= 16 else (8, 24), items=items)


def c32_accepts(B, H, W, sh):
    """what asr_conv7x7c32_supported must answer: all three launchers take the shape"""
    return all(plan(op, (B, H, W, sh)) is not None for op in ('c32_fwd', 'c32_dgrad', 'c32_wgrad'))


def c1_accepts(Fw, cin):
    """what asr_conv1_7x7s2_supported must answer"""
    if Fw < KS or cin not in (1, 3):
        return False
    ops = ('c1_fwd', 'c1_wgrad') if cin == 1 else ('c1c_fwd', 'c1c_wgrad')
    return all(plan(op, (1, 1, Fw)) is not None for op in ops)


# ------------------------------------------------------------------ the matrix

# (B, H, W) of the 32 -> 32 convolution at stride 3.  With Wo = W - 6:
#   forward          R  = min(16, FWD_PIX / Wo) output rows per item (FWD_PIX = 128 = 4 MFMA tiles)
#   input gradient   Rq = min(16, DG_PIX / W) rows per class and item (DG_PIX = 192), nq = ceil(H / 3)
#   weight gradient  KW = ceil(Wo / 16) k-steps per row, `rows` = 8, 4 or 2 output rows per chunk:
#                    the most with (3 (rows - 1) + 7) * W * 4 <= NX_MAX * WGRAD_NT = 3584 staging
#                    slots and rows * 16 KW * 4 <= ND_MAX * WGRAD_NT = 1344: 8 up to W = 22 (the
#                    dy slots: KW = 2 from W = 23 on), 4 up to W = 44 (the x slots), then 2
# tests/test_conv_referee.py::test_matrix_straddles_the_constants derives all of this from `plan`
# and fails if a constant moves
C32_SHAPES = [
    ('w7', (2, 490, 7)),         # Wo = 1: R = Rq = 16 (the caps), Ho = 162: Ho % R = 2
    ('w13', (6, 31, 13)),        # Wo = 7: R * Wo = 126, not a multiple of 32
    ('w17', (2, 58, 17)),        # the benchmark width: R = 11 (121 pixels), Ho = 18 % 11; nq = 20 % Rq = 11
    ('w17_h59', (2, 59, 17)),    # (H - 7) % 3 = 1: one trailing input row no window covers
    ('w17_h60', (2, 60, 17)),    # (H - 7) % 3 = 2: two
    ('w17_h7', (30, 7, 17)),     # Ho = 1 < R; three q rows < Rq
    ('w22', (2, 40, 22)),        # Wo = 16: KW = 1, the last width with 8 weight-gradient rows per chunk
    ('w23', (2, 40, 23)),        # Wo = 17: KW = 2, 4 rows per chunk: Ho = 12 makes three chunks
    ('w38', (2, 64, 38)),        # the WSJ width, Wo = 32: KW = 2
    ('w39', (2, 40, 39)),        # Wo = 33: KW = 3
    ('w44', (2, 40, 44)),        # the last width with 4 weight-gradient rows per chunk
    ('w45', (2, 43, 45)),        # 2 rows per chunk; Ho = 13: a last chunk of one row
    ('w48', (2, 40, 48)),        # the widest: Wo = 42, R = 3, Rq = 4
    # persistent loops: 171 x 3 = 513 forward and input-gradient items against 2 x 256
    # workgroups (a second item for workgroup 0; the input gradient's `flip` roles), 513
    # weight-gradient chunks against WGRAD_WGS = 256
    ('persist', (171, 31, 48)),
]
C32_S1_SHAPES = [('s1_w7', (320, 7, 7)), ('s1_w13', (3, 31, 13)), ('s1_w48', (2, 20, 48))]

# (B, T, F) of the one-channel first convolution: Fo = (F - 7) / 2 + 1, To = T + 6, 16 rows per
# chunk.  Weight-gradient prefetch templates <DI, WPT>, DI = ceil(Fo / 4), WPT = ceil(24 Fo / 256):
# <5, 2> up to Fo = 20, <8, 3> up to 32, <16, 6> up to Fo = 39 (F = 84), the widest both kernels take
C1_SHAPES = [
    ('f7', (4, 75, 7)),          # Fo = 1; To = 81: a last chunk of ONE row
    ('f9', (3, 50, 9)),
    ('f40', (2, 50, 40)),        # the benchmark features, <5, 2>; To = 56: To % 16 = 8
    ('f40_t1', (8, 1, 40)),      # T = 1: every output row reads the padding
    ('f40_t11', (2, 11, 40)),    # To = 17: a last chunk of one row
    ('f46', (2, 20, 46)),        # Fo = 20: the last <5, 2> width (an even F: the window of the
                                 # last column ends on the row's last sample)
    ('f47', (2, 20, 47)),        # Fo = 21: <8, 3>
    ('f53', (2, 30, 53)),
    ('f69', (2, 20, 69)),        # Fo = 32: the last <8, 3> width
    ('f71', (2, 20, 71)),        # Fo = 33: <16, 6>
    ('f81', (3, 33, 81)),
    ('f84', (2, 20, 84)),        # Fo = 39: the widest
    ('persist', (1030, 10, 21)),  # 1030 one-chunk utterances against C1_WGS = 1024 workgroups
]
# three channels: even Fo only, 8 rows per chunk; RPT = 16 up to F = 85, 24 at F = 86 (Fo = 40,
# the widest both kernels take)
C1C_SHAPES = [
    ('f9', (40, 2, 9)),          # Fo = 2, To = 8: To % 8 = 0
    ('f49_t3', (3, 3, 49)),      # To = 9: To % 8 = 1
    ('f49_t9', (3, 9, 49)),      # To = 15: To % 8 = 7
    ('f81', (2, 50, 81)),        # the WSJ features
    ('f85', (2, 20, 85)),        # the last RPT = 16 width
    ('f86', (2, 20, 86)),        # RPT = 24
    ('persist', (1030, 2, 9)),   # 1030 chunks against 768 forward and C1_WGS = 1024 weight-gradient workgroups
]


def cases():
    out = []
    for name, (B, H, W) in C32_SHAPES:
        for op in ('c32_fwd', 'c32_dgrad', 'c32_wgrad'):
            out.append(dict(op=op, name=name, shape=(B, H, W, 3)))
    for name, (B, H, W) in C32_S1_SHAPES:
        out.append(dict(op='c32_fwd', name=name, shape=(B, H, W, 1)))
    for ops, shapes in ((('c1_fwd', 'c1_wgrad'), C1_SHAPES), (('c1c_fwd', 'c1c_wgrad'), C1C_SHAPES)):
        for name, shape in shapes:
            for op in ops:
                out.append(dict(op=op, name=name, shape=shape))
    return out


def case_id(case):
    return '%s-%s' % (case['op'], case['name'])


def geometry(case):
    """(cin, x shape, w shape, y shape, stride, padding) in logical layout"""
    op, s = case['op'], case['shape']
    if op.startswith('c32'):
        B, H, W, sh = s
        return 32, (B, 32, H, W), (32, 32, 7, 7), (B, 32, (H - 7) // sh + 1, W - 6), (sh, 1), (0, 0)
    cin = 1 if op.startswith('c1_') else 3
    B, T, Fw = s
    return cin, (B, cin, T, Fw), (32, cin, 7, 7), (B, 32, T + 6, (Fw - 7) // 2 + 1), (1, 2), (6, 0)


def products(case):
    """K: the number of products in one output element's sum"""
    cin, xs, ws, ys, _, _ = geometry(case)
    if case['op'].endswith('wgrad'):
        return ys[0] * ys[2] * ys[3]
    return 49 * cin


def tensor_bytes(case):
    """device bytes of the largest tensor of the case"""
    cin, xs, ws, ys, _, _ = geometry(case)
    xb = int(np.prod(xs)) * (2 if case['op'].startswith('c32') else 4)
    return max(xb, int(np.prod(ys)) * 2)


# ------------------------------------------------------------------ operands

def _seed(case, salt):
    return (hash_name(case_id(case)) + salt) & 0x7fffffff


def hash_name(s):
    h = 2166136261
    for c in s.encode():
        h = ((h ^ c) * 16777619) & 0xffffffff
    return h


def _sparse_ints(g, shape, density):
    v = torch.randint(1, 3, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    return v * (torch.rand(shape, generator=g, dtype=torch.float64) < density)


def integer_density(case):
    """density of the nonzero activations (features for conv1).  The recipe's 1/8 (1/2 for the
    conv1 features), halved while the EXPECTED sum(y^2) of a forward case exceeds 2^23, so that
    the channel sums stay exactly representable in every fp32 partial order (judge); not below
    1/64 (1/8 for conv1), where the large persistent cases fall back to the 1e-5 comparison.
    Expectations from the recipe: a nonzero operand is +-1 or +-2 (mean square 2.5); the 32 -> 32
    weights have density 1/2, the dense conv1 weights are uniform in {-2..2} (mean square 2)."""
    op = case['op']
    cin, xs, ws, ys, _, _ = geometry(case)
    c32 = op.startswith('c32')
    d, floor = (1 / 8, 1 / 64) if c32 else (1 / 2, 1 / 8)
    if op in FWD:
        per = 49 * cin * 2.5 * (1.25 if c32 else 2.0)
        while d > floor and int(np.prod(ys)) * per * d > 2 ** 23:
            d /= 2
    return d


def integer_inputs(case):
    """x (features), w and dy as float64 tensors of small integers, all exact in bf16"""
    op = case['op']
    cin, xs, ws, ys, _, _ = geometry(case)
    g = torch.Generator().manual_seed(_seed(case, 1))
    x = _sparse_ints(g, xs, integer_density(case))
    if op.startswith('c32'):
        w = _sparse_ints(g, ws, 1 / 2)
    else:
        w = torch.randint(-2, 3, ws, generator=g).double()
    dy = _sparse_ints(g, ys, 1 / 8)
    return dict(x=x, w=w, dy=dy, kind='integer')


def gaussian_inputs(case):
    """the operands of tests/test_conv_gpu.py: unit Gaussians, weights x 0.05 (x 0.1 for conv1)"""
    op = case['op']
    cin, xs, ws, ys, _, _ = geometry(case)
    g = torch.Generator().manual_seed(_seed(case, 2))
    x = torch.randn(xs, generator=g)
    w = torch.randn(ws, generator=g) * (0.05 if op.startswith('c32') else 0.1)
    dy = torch.randn(ys, generator=g)
    return dict(x=x.double(), w=w.double(), dy=dy.double(), kind='gaussian')


def rounded(inp):
    """the operands as the kernels see them: bf16, round to nearest even (the packing kernels
    round the fp32 weights, the conv1 kernels the fp32 features), as float64"""
    return {k: v.float().to(torch.bfloat16).double() for k, v in inp.items() if k != 'kind'}


# ------------------------------------------------------------------ reference

def _conv(case, x, w, dy):
    """the case's operation on tensors of one dtype"""
    op = case['op']
    cin, xs, ws, ys, stride, pad = geometry(case)
    if op in FWD:
        return F.conv2d(x, w, None, stride, pad)
    if op == 'c32_dgrad':
        return torch.nn.grad.conv2d_input(xs, w, dy, stride=stride, padding=pad)
    return torch.nn.grad.conv2d_weight(x, ws, dy, stride=stride, padding=pad)


def ulp_bf16(v):
    """the spacing of bf16 at |v| (2^-133, the smallest subnormal's, at 0)"""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.ldexp(1.0, np.maximum(e - 8, -133))


def bf16_round(a, truncate=False):
    """float32 array -> the bf16 values, as float64"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if truncate:
        return (t.view(torch.int32) & -65536).view(torch.float32).double().numpy()
    return t.to(torch.bfloat16).double().numpy()


def _stats(case, got, want, S):
    """(rounding bias, RMS) of got against want in bf16 ulps of want, over the covered elements"""
    m = S > 0
    u = (got[m] - want[m]) / ulp_bf16(want[m])
    return float(np.mean(np.sign(want[m]) * u)), float(np.sqrt(np.mean(u * u))), int(m.sum())


def reference(case, inp):
    """dict(out fp64, S, sums [2, 32] of the outputs (forward), and on Gaussian operands out32 (the
    fp32 CPU convolution) with rms32, the RMS statistic of bf16_rne(out32))"""
    r = rounded(inp)
    out = _conv(case, r['x'], r['w'], r['dy']).numpy()
    S = _conv(case, r['x'].abs(), r['w'].abs(), r['dy'].abs()).numpy()
    want = dict(out=out, S=S)
    if inp['kind'] == 'integer':
        lim = 128 if case['op'] in BF16_OUT else 2 ** 24 - 1
        assert np.abs(out).max() <= lim, (case_id(case), float(np.abs(out).max()))
        assert np.array_equal(out, np.rint(out))
    else:
        want['out32'] = _conv(case, r['x'].float(), r['w'].float(), r['dy'].float()).numpy()
        if case['op'] in BF16_OUT:
            want['bias32'], want['rms32'], want['n'] = _stats(case, bf16_round(want['out32']), out, S)
    if case['op'] in FWD:
        yb = out if inp['kind'] == 'integer' else bf16_round(out.astype(np.float32))
        want['sums'] = np.stack([yb.sum((0, 2, 3)), (yb * yb).sum((0, 2, 3))])
        want['sumsq_total'] = float((yb * yb).sum())
    return want


# ------------------------------------------------------------------ judge

def _where(bad, n=4):
    idx = np.argwhere(bad)
    return '%d elements, first at (b, channel, row, column) %s' % (len(idx), [tuple(int(i) for i in r) for r in idx[:n]])


def judge(case, got, want, kind, stats=None):
    """complaints about got = dict(out=<fp64 array, logical layout>, sums=<[2, 32] or None>)"""
    op, bad = case['op'], []
    out, ref, S = np.asarray(got['out'], np.float64), want['out'], want['S']
    if out.shape != ref.shape:
        return ['shape %s, want %s' % (out.shape, ref.shape)]
    if kind == 'integer':
        ne = ~(out == ref)                                  # (a NaN is a mismatch)
        if ne.any():
            bad.append('%s: %s' % (op, _where(ne)))
    else:
        K = products(case)
        r = 0.5 * ulp_bf16(ref) if op in BF16_OUT else 2.0 ** -23 * np.abs(ref)
        over = ~(np.abs(out - ref) <= r + K * 2.0 ** -23 * S)
        if stats is not None:
            with np.errstate(divide='ignore', invalid='ignore'):
                share = np.abs(out - ref) / (r + K * 2.0 ** -23 * S)
            stats['share'] = float(np.nanmax(np.where(S > 0, share, 0.0)))
        if over.any():
            bad.append('%s per-element bound: %s' % (op, _where(over)))
        if op in BF16_OUT:
            bias, rms, n = _stats(case, out, ref, S)
            if stats is not None:
                stats.update(bias=bias, rms=rms, rms32=want['rms32'], n=n)
            if n < 10 ** 4:
                bad.append('%s: %d covered elements, the statistics need 10^4' % (op, n))
            if not abs(bias) <= 0.02:
                bad.append('%s rounding bias %.4f ulp (round-to-nearest: 0, truncation: -0.5)' % (op, bias))
            if not rms <= 1.05 * want['rms32']:
                bad.append('%s RMS error %.4f ulp, %.4f for bf16(fp32 convolution)' % (op, rms, want['rms32']))
    if op in FWD and got.get('sums') is not None:
        sums = np.asarray(got['sums'], np.float64)
        if kind == 'integer' and want['sumsq_total'] < 2 ** 24:
            if not np.array_equal(sums, want['sums']):
                bad.append('%s channel sums differ from the exact ones at %s' % (op, np.argwhere(sums != want['sums'])[:4].tolist()))
        else:
            own = np.stack([out.sum((0, 2, 3)), (out * out).sum((0, 2, 3))])
            if not (np.allclose(sums[0], own[0], rtol=1e-5, atol=1e-3) and np.allclose(sums[1], own[1], rtol=1e-5)):
                bad.append('%s channel sums are not those of the outputs' % op)
    return bad


# ------------------------------------------------------------------ model

def poison(case):
    return float(torch.tensor([POISON_H], dtype=torch.int16).view(torch.bfloat16).double()) \
        if case['op'] in BF16_OUT else POISON_F


def applies(case, mut):
    """whether the mutant changes anything at this case"""
    op, pl = case['op'], plan(case['op'], case['shape'])
    cin, xs, ws, ys, stride, pad = geometry(case)
    if mut in ('tap66_dropped',):
        return True
    if mut == 'last_column_unwritten':
        return op in BF16_OUT
    if mut == 'partial_block_last_row_unwritten':
        if op == 'c32_fwd':
            return pl['Ho'] % pl['R'] != 0
        if op == 'c32_dgrad':
            return pl['nq'] % pl['Rq'] != 0
        return op in FWD and pl['To'] % pl['rows'] != 0
    if mut == 'ci_30_31_swapped':
        return op.startswith('c32')
    if mut == 'dgrad_class2_dropped':
        return op == 'c32_dgrad'
    if mut == 'dx_trailing_rows_unwritten':
        return op == 'c32_dgrad' and (xs[2] - 7) % 3 != 0
    if mut == 'bf16_truncated':
        return op in BF16_OUT
    if mut == 'acc_bf16_every_16':
        return op in ('c32_fwd', 'c1_fwd') and int(np.prod(ys)) <= 40000
    if mut == 'sums_miss_last_group':
        return op in FWD
    if mut == 'wgrad_misses_last_chunk':
        return op.endswith('wgrad')
    raise KeyError(mut)


def _acc_bf16_every_16(case, x, w):
    """the forward sum in the kernels' k order (tap row, tap column, channel), the running sum
    rounded to bf16 after every 16 products"""
    cin, xs, ws, ys, stride, pad = geometry(case)
    xp = F.pad(x, (pad[1], pad[1], pad[0], pad[0]))
    Ho, Wo = ys[2], ys[3]
    acc = torch.zeros(ys, dtype=torch.float32)
    n = 0
    for kt in range(7):
        for kf in range(7):
            win = xp[:, :, kt:kt + stride[0] * (Ho - 1) + 1:stride[0], kf:kf + stride[1] * (Wo - 1) + 1:stride[1]]
            for c0 in range(0, cin, 16):
                acc = acc + torch.einsum('bchw,oc->bohw', win[:, c0:c0 + 16], w[:, c0:c0 + 16, kt, kf])
                n += min(16, cin - c0)
                if n >= 16:
                    acc, n = acc.to(torch.bfloat16).float(), 0
    return acc


def model(case, inp, mut=None):
    """got = dict(out, sums): the operation in fp32 on the rounded operands, bf16 outputs rounded
    to nearest even — with `mut`, one wrong term"""
    op, pl = case['op'], plan(case['op'], case['shape'])
    cin, xs, ws, ys, stride, pad = geometry(case)
    assert mut is None or applies(case, mut)
    r = {k: v.float() for k, v in rounded(inp).items()}
    x, w, dy = r['x'], r['w'], r['dy']
    if mut == 'tap66_dropped' and not op.endswith('wgrad'):
        w = w.clone()
        w[:, :, 6, 6] = 0
    if mut == 'ci_30_31_swapped' and op != 'c32_dgrad':
        x = x[:, list(range(30)) + [31, 30]]
    if mut == 'wgrad_misses_last_chunk':
        dy = dy.clone()
        last = (ys[2] - 1) // pl['rows'] * pl['rows']
        dy[-1, :, last:] = 0
    if mut == 'acc_bf16_every_16':
        acc = _acc_bf16_every_16(case, x, w)
    else:
        acc = _conv(case, x, w, dy)
    if mut == 'tap66_dropped' and op.endswith('wgrad'):
        acc[:, :, 6, 6] = 0
    if mut == 'ci_30_31_swapped' and op == 'c32_dgrad':
        acc = acc[:, list(range(30)) + [31, 30]]
    if mut == 'dgrad_class2_dropped':
        acc[:, :, 2::3] = 0
    out = bf16_round(acc.numpy(), truncate=mut == 'bf16_truncated') if op in BF16_OUT else acc.double().numpy()
    sums = None
    if op in FWD:
        sums = np.stack([out.sum((0, 2, 3)), (out * out).sum((0, 2, 3))])
        if mut == 'sums_miss_last_group':      # the last 8 pixels of the last utterance
            tail = out[-1].reshape(32, -1)[:, -8:]
            sums = sums - np.stack([tail.sum(1), (tail * tail).sum(1)])
    if mut == 'last_column_unwritten':
        out[..., -1] = poison(case)
    if mut == 'partial_block_last_row_unwritten':
        out[:, :, -1] = poison(case)
    if mut == 'dx_trailing_rows_unwritten':
        out[:, :, 3 * (ys[2] - 1) + 7:] = poison(case)
    return dict(out=out, sums=sums)
