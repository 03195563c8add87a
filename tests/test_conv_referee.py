"""The referee of the convolution kernels (tests/conv_referee.py) is proved here before it judges
a kernel in tests/test_conv_referee_gpu.py; nothing in this file needs a GPU.

* The matrix is what it claims: unique cases, every op, no tensor above 32 MB, every case taken by
  its launcher, at least 10^4 covered elements where the rounding statistics are taken, and the
  shapes on both sides of each constant of csrc/conv.hip that `cases()` names.
* The integer recipe meets its range condition at every case (`reference` asserts it).
* The unmutated model passes the integer and the Gaussian judge at every case.
* Every mutant is rejected at every case it applies to:
    tap66_dropped                      integer judge, 85 cases (every op)
    last_column_unwritten              integer and Gaussian, the 51 cases with a bf16 output
    partial_block_last_row_unwritten   integer and Gaussian, 42 cases (Ho % R, nq % Rq, To % rows != 0)
    ci_30_31_swapped                   integer and Gaussian, the 45 cases of the 32 -> 32 convolution
    dgrad_class2_dropped               integer and Gaussian, the 14 input-gradient cases
    dx_trailing_rows_unwritten         integer and Gaussian, c32_dgrad-w17_h59 and -w17_h60
    bf16_truncated                     Gaussian judge (rounding bias -0.5), 51 cases; integers are
                                       exact either way
    acc_bf16_every_16                  Gaussian judge (per-element bound and RMS), the 21 forward
                                       cases of at most 40000 outputs it is evaluated at
    sums_miss_last_group               integer and Gaussian, the 37 forward cases
    wgrad_misses_last_chunk            integer judge, 34 cases; the Gaussian judge passes it at
                                       c32_wgrad-persist and c1_wgrad-persist, where one chunk of
                                       513 / 1030 lies below the K 2^-23 S allowance
  (the Gaussian judge also passes tap66_dropped at c1_wgrad-persist for the same reason: the
  integer data is what catches a missing term of a long sum.)
* The gate sweep: the Python gates, the library's queries and the referee's port of the launchers'
  arithmetic agree at every width.

The accumulation-precision rule compares with the RMS error, in bf16 ulps, of bf16_rne(fp32 CPU
convolution) against the fp64 reference.  Measured per case (near 1 / sqrt(12) = 0.2887; at
c32_dgrad-w38 one element with |want| far below its S carries the statistic):
  c32_fwd: w7 0.2892, w13 0.2902, w17 0.2873, w17_h59 0.2898, w17_h60 0.2887, w17_h7 0.2862, w22
    0.2886, w23 0.2878, w38 0.2887, w39 0.2979, w44 0.2905, w45 0.2881, w48 0.2885, persist 0.2918,
    s1_w7 0.2879, s1_w13 0.2886, s1_w48 0.2892
  c32_dgrad: w7 0.2885, w13 0.2889, w17 0.2896, w17_h59 0.2893, w17_h60 0.2887, w17_h7 0.2889, w22
    0.2894, w23 0.2886, w38 0.4325, w39 0.2886, w44 0.2889, w45 0.2886, w48 0.2890, persist 0.2889
  c1_fwd: f7 0.2893, f9 0.2885, f40 0.2885, f40_t1 0.2888, f40_t11 0.2899, f46 0.2881, f47 0.2888,
    f53 0.2880, f69 0.2889, f71 0.2900, f81 0.2889, f84 0.2887, persist 0.2904
  c1c_fwd: f9 0.2873, f49_t3 0.2877, f49_t9 0.2886, f81 0.2882, f85 0.2883, f86 0.2887, persist
    0.2888"""
import functools

import numpy as np
import pytest

import conv_referee as cr

CASES = cr.cases()
IDS = [cr.case_id(c) for c in CASES]
BY_ID = dict(zip(IDS, CASES))
# mutants only one of the two judges can see
INTEGER_ONLY = {('wgrad_misses_last_chunk', 'c32_wgrad-persist'), ('wgrad_misses_last_chunk', 'c1_wgrad-persist'),
                ('tap66_dropped', 'c1_wgrad-persist')}
ROUNDING = ('bf16_truncated', 'acc_bf16_every_16')


@functools.lru_cache(maxsize=None)
def prepared(cid, kind):
    case = BY_ID[cid]
    inp = cr.integer_inputs(case) if kind == 'integer' else cr.gaussian_inputs(case)
    return inp, cr.reference(case, inp)


def test_matrix_is_what_it_claims():
    assert len(set(IDS)) == len(IDS)
    assert len({(c['op'], c['shape']) for c in CASES}) == len(CASES)
    assert {c['op'] for c in CASES} == set(cr.OPS)
    assert {c['shape'][3] for c in CASES if c['op'] == 'c32_fwd'} == {1, 3}
    for c in CASES:
        assert cr.tensor_bytes(c) <= 32 * 2 ** 20, cr.case_id(c)
        assert cr.plan(c['op'], c['shape']) is not None, cr.case_id(c)


def _p(op, name):
    c = BY_ID['%s-%s' % (op, name)]
    return cr.plan(op, c['shape'])


def test_matrix_straddles_the_constants():
    """the boundaries `cases()` names in its comments, derived from the port of the launchers"""
    # forward: the row cap, a pixel count that is no multiple of the 32-pixel tile, Ho < R, Ho % R
    assert _p('c32_fwd', 'w7')['R'] == 16 and _p('c32_fwd', 'w7')['Ho'] % 16 == 2
    for name in ('w13', 'w17'):
        p = _p('c32_fwd', name)
        assert (p['R'] * p['Wo']) % 32 != 0
    assert _p('c32_fwd', 'w17_h7')['Ho'] == 1 < _p('c32_fwd', 'w17_h7')['R']
    assert _p('c32_fwd', 'w17')['Ho'] % _p('c32_fwd', 'w17')['R'] != 0
    assert _p('c32_fwd', 'w48')['R'] == 3 and _p('c32_dgrad', 'w48')['Rq'] == 4
    # input gradient: nq % Rq != 0, and every count of trailing rows
    assert _p('c32_dgrad', 'w17')['nq'] % _p('c32_dgrad', 'w17')['Rq'] != 0
    assert {(BY_ID['c32_dgrad-' + n]['shape'][1] - 7) % 3 for n in ('w17', 'w17_h59', 'w17_h60')} == {0, 1, 2}
    # weight gradient: KW at Wo = 16 | 17 and 32 | 33, rows per chunk 8 | 4 | 2
    assert [_p('c32_wgrad', n)['KW'] for n in ('w22', 'w23', 'w38', 'w39')] == [1, 2, 2, 3]
    assert [_p('c32_wgrad', n)['rows'] for n in ('w22', 'w23', 'w44', 'w45')] == [8, 4, 4, 2]
    assert _p('c32_wgrad', 'w45')['Ho'] % 2 == 1
    # persistent loops: more items than the 2 x 256 workgroups of an MI355X / than WGRAD_WGS
    assert _p('c32_fwd', 'persist')['items'] == _p('c32_dgrad', 'persist')['items'] == 513
    assert _p('c32_wgrad', 'persist')['items'] > cr.WGRAD_WGS
    assert _p('c1_wgrad', 'persist')['items'] > cr.C1_WGS and _p('c1c_wgrad', 'persist')['items'] > cr.C1_WGS
    assert _p('c1c_fwd', 'persist')['items'] > cr.C1C_FWD_WGS
    # conv1: the prefetch template classes on both sides of each edge, the row edges
    assert [_p('c1_wgrad', n)['cls'] for n in ('f46', 'f47', 'f69', 'f71', 'f84')] == [
        (5, 2), (8, 3), (8, 3), (16, 6), (16, 6)]
    assert cr.plan('c1_wgrad', (1, 1, 85)) is None and cr.plan('c1_fwd', (1, 1, 85)) is not None
    assert {_p('c1_fwd', n)['To'] % 16 for n in ('f7', 'f40_t11')} == {1}
    assert _p('c1_fwd', 'f40_t1')['To'] == 7
    assert [_p('c1c_fwd', n)['rpt'] for n in ('f85', 'f86')] == [16, 24]
    assert [_p('c1c_wgrad', n)['cls'] for n in ('f85', 'f86')] == [(5, 16), (8, 24)]
    assert {_p('c1c_fwd', n)['To'] % 8 for n in ('f9', 'f49_t3', 'f49_t9')} == {0, 1, 7}
    assert cr.plan('c1c_wgrad', (1, 1, 89)) is None


@pytest.mark.parametrize('cid', IDS)
def test_integer_recipe_and_unmutated_model(cid):
    """`reference` asserts the range condition of the integer operands; the model passes both judges"""
    case = BY_ID[cid]
    for kind in ('integer', 'gaussian'):
        inp, want = prepared(cid, kind)
        stats = {}
        bad = cr.judge(case, cr.model(case, inp), want, kind, stats)
        assert not bad, bad
        if kind == 'gaussian' and case['op'] in cr.BF16_OUT:
            assert stats['n'] >= 10 ** 4
    inp, want = prepared(cid, 'integer')
    assert np.abs(want['out']).max() > 0
    if case['op'] in cr.FWD and case['name'] != 'persist':
        assert want['sumsq_total'] < 2 ** 24        # the channel sums are judged exactly


@pytest.mark.parametrize('mut', cr.MUTANTS)
def test_mutant_is_rejected(mut):
    seen = 0
    for cid in IDS:
        case = BY_ID[cid]
        if not cr.applies(case, mut):
            continue
        seen += 1
        kinds = ('gaussian',) if mut in ROUNDING else (
            ('integer',) if (mut, cid) in INTEGER_ONLY else ('integer', 'gaussian'))
        for kind in kinds:
            inp, want = prepared(cid, kind)
            assert cr.judge(case, cr.model(case, inp, mut), want, kind), (mut, cid, kind)
    assert seen >= 2


# ------------------------------------------------------------------ gates

class _Shape:
    """what native_conv.supported / first_supported ask of a tensor"""
    is_cuda, requires_grad = True, False

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)

    def size(self, i):
        return self.shape[i]


def _gates():
    import torch
    from att_speech import _native
    from att_speech.modules.encoders import native_conv
    _native.lib()
    conv2 = {sh: torch.nn.Conv2d(32, 32, (7, 7), stride=(sh, 1)) for sh in (1, 3)}
    conv1 = {cin: torch.nn.Conv2d(cin, 32, (7, 7), stride=(1, 2), padding=(6, 0)) for cin in (1, 3)}

    def second(B, H, W, sh):
        return bool(native_conv.supported(conv2[sh], _Shape(B, 32, H, W)))

    def first(Fw, cin):
        return bool(native_conv.first_supported(conv1[cin], _Shape(2, cin, 50, Fw)))
    return _native, second, first


def test_gate_sweep_second_convolution():
    """every width at both strides: the gate the encoder asks, the library's query and the port"""
    N, second, _ = _gates()
    L = N.lib()
    for W in range(7, 65):
        for sh in (1, 3):
            q = bool(L.asr_conv7x7c32_supported(2, 40, W, sh))
            assert q == cr.c32_accepts(2, 40, W, sh), (W, sh)
            assert N.conv7x7c32_supported(2, 40, W, sh) == q, (W, sh)
            # (the encoder's convolution has stride 3; the stride-1 forward has no gradient kernels)
            assert second(2, 40, W, sh) == (q and sh == 3), (W, sh)
    # the limits include/asr_amd.h and the README state
    assert [W for W in range(7, 65) if not L.asr_conv7x7c32_supported(2, 40, W, 3)] == [12, 14, 15, 20] + list(range(49, 65))
    assert not any(L.asr_conv7x7c32_supported(2, 40, W, 1) for W in range(7, 65))
    assert all(cr.plan('c32_fwd', (2, 40, W, 1)) is not None for W in range(7, 55))
    assert not L.asr_conv7x7c32_supported(2, 6, 17, 3) and not L.asr_conv7x7c32_supported(0, 40, 17, 3)


# one shape on each side of the 32-bit byte-offset limits: H * W * 64 < 2^31 (forward) and
# B * Ho * Wo * 64 < 2^31 (input gradient; Ho = 18, Wo = 11)
OFFSET_LIMITS = [((1, 1973790, 17), True), ((1, 1973791, 17), False),
                 ((169466, 58, 17), True), ((169467, 58, 17), False)]


@pytest.mark.parametrize('shape,ok', OFFSET_LIMITS)
def test_gate_at_the_offset_limits(shape, ok):
    N, second, _ = _gates()
    B, H, W = shape
    assert (H * W * 64 < 2 ** 31 and B * ((H - 7) // 3 + 1) * (W - 6) * 64 < 2 ** 31) == ok
    assert bool(N.lib().asr_conv7x7c32_supported(B, H, W, 3)) == ok
    assert cr.c32_accepts(B, H, W, 3) == ok
    assert second(B, H, W, 3) == ok


def test_gate_sweep_first_convolution():
    N, _, first = _gates()
    L = N.lib()
    for Fw in range(7, 201):
        for cin in (1, 3):
            q = bool(L.asr_conv1_7x7s2_supported(Fw, cin))
            assert q == cr.c1_accepts(Fw, cin), (Fw, cin)
            assert N.conv1_supported(Fw, cin) == q and first(Fw, cin) == q, (Fw, cin)
    # the limits include/asr_amd.h and the README state: Fo <= 39, and even Fo <= 40
    assert [Fw for Fw in range(1, 201) if N.conv1_supported(Fw, 1)] == list(range(7, 85))
    assert [Fw for Fw in range(1, 201) if N.conv1_supported(Fw, 3)] == [
        Fw for Fw in range(7, 87) if ((Fw - 7) // 2 + 1) % 2 == 0]
    assert not N.conv1_supported(40, 2) and not L.asr_conv1_7x7s2_supported(40, 2)
    # the fused weight gradient is built for a subset of the supported widths
    assert all(N.conv1_supported(Fw, 1) for Fw in range(7, 201) if N.conv1_wgrad_bn_supported(Fw))
