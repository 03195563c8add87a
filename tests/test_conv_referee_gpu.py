"""The convolution kernels of csrc/conv.hip against tests/conv_referee.py, one launch at a time.

The C entry points themselves are called (through _native.lib()), not the _native wrappers: the
wrappers allocate their outputs with torch.empty, and the caching allocator can hand back a block
that still holds the right answer of the previous call, which would hide an element a kernel never
wrote.  Here every output is pre-filled with a poison pattern, sits between two poisoned guard
zones that must come back untouched, and every input sits between two guard zones of NaNs: an
input element read from beyond its tensor and multiplied into a sum shows in the output.  The
workspace starts as all-ones bits (NaN as fp32) for the same reason.

Per case the integer operands are judged first (every element equal to the fp64 reference, the
channel sums too), then the Gaussian ones (per-element bound, rounding bias, accumulation
precision: conv_referee.judge).  tests/test_conv_referee.py proves the judges on the CPU.

What the NaN guards found when this file was written: at an odd feature count F the one-channel
forward kernel read the 8th sample of a row's last window from behind the row — for the last row
of the last utterance from behind the tensor — and multiplied it with its zero weight.  With a
NaN there, c1_fwd-f7 came back with NaNs in the last column of the 8 output rows that touch the
last input row (256 elements, first at (3, 0, 73, 0)); conv1_stage_windows no longer loads it."""
import numpy as np
import pytest
import torch

import conv_referee as cr

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GUARD = 256                         # elements on each side of a tensor
CASES = cr.cases()


def native():
    from att_speech import _native
    _native.lib()
    return _native


def guarded(shape, dtype, fill):
    """(tensor of `shape` inside a flat buffer, the buffer): both filled with `fill` (bits for bf16)"""
    n = int(np.prod(shape))
    if dtype == torch.bfloat16:
        buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    else:
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(shape), buf


def guards_intact(buf, dtype, fill):
    bits = buf.view(torch.int16) if dtype == torch.bfloat16 else buf
    ends = torch.cat([bits[:GUARD], bits[-GUARD:]])
    return bool((ends == torch.full_like(ends, fill)).all())


NAN_H = 0x7fc0


def nhwc_in(t):
    """logical [B, C, H, W] float64 -> bf16 channels-last memory between NaN guards, logical view"""
    B, C, H, W = t.shape
    mem, _ = guarded((B, H, W, C), torch.bfloat16, NAN_H)
    mem.copy_(t.permute(0, 2, 3, 1).to(torch.bfloat16))
    return mem


def f32_in(t):
    mem, _ = guarded(tuple(t.shape), torch.float32, float('nan'))
    mem.copy_(t.float())
    return mem


def nhwc_out(shape):
    B, C, H, W = shape
    return guarded((B, H, W, C), torch.bfloat16, cr.POISON_H)


def logical(mem):
    """channels-last bf16 memory [B, H, W, C] -> logical [B, C, H, W] float64 on the host"""
    return mem.permute(0, 3, 1, 2).float().cpu().double().numpy()


def workspace(nbytes):
    return torch.full((nbytes,), 0xff, dtype=torch.uint8, device=DEV)


def launch(case, inp):
    """one call of the case's entry point on poisoned outputs -> got for conv_referee.judge"""
    N = native()
    L, p, st = N.lib(), N._p, N._stream()
    op = case['op']
    cin, xs, ws_, ys, stride, pad = cr.geometry(case)
    sums = sums_buf = None
    if op in cr.FWD:
        sums, sums_buf = guarded((2, 32), torch.float64, cr.POISON_F)
    w = f32_in(inp['w'])
    if op.startswith('c32'):
        B, H, W, sh = case['shape']
        nbytes = L.asr_conv7x7c32_workspace_bytes()
        ws = workspace(nbytes)
        if op == 'c32_fwd':
            x = nhwc_in(inp['x'])
            out, buf = nhwc_out(ys)
            rc = L.asr_conv7x7c32_fwd_bf16(p(x), p(w), B, H, W, sh, p(out), p(sums), p(ws), nbytes, st)
        elif op == 'c32_dgrad':
            dy = nhwc_in(inp['dy'])
            out, buf = nhwc_out(xs)
            rc = L.asr_conv7x7c32_bwd_data_bf16(p(dy), p(w), B, H, W, sh, p(out), p(ws), nbytes, st)
        else:
            x, dy = nhwc_in(inp['x']), nhwc_in(inp['dy'])
            out, buf = guarded(ws_, torch.float32, cr.POISON_F)
            rc = L.asr_conv7x7c32_wgrad_bf16(p(x), p(dy), B, H, W, sh, p(out), p(ws), nbytes, st)
    else:
        B, T, Fw = case['shape']
        x = f32_in(inp['x'][:, 0] if cin == 1 else inp['x'].permute(0, 2, 3, 1))     # [B, T, F(, cin)]
        nbytes = L.asr_conv1_7x7s2_workspace_bytes() if cin == 1 else L.asr_conv1c_7x7s2_workspace_bytes(cin)
        ws = workspace(nbytes)
        if op in cr.FWD:
            out, buf = nhwc_out(ys)
            if cin == 1:
                rc = L.asr_conv1_7x7s2_fwd(p(x), p(w), B, T, Fw, p(out), p(sums), p(ws), nbytes, st)
            else:
                rc = L.asr_conv1c_7x7s2_fwd(p(x), p(w), B, T, Fw, cin, p(out), p(sums), p(ws), nbytes, st)
        else:
            dy = nhwc_in(inp['dy'])
            out, buf = guarded(ws_, torch.float32, cr.POISON_F)
            if cin == 1:
                rc = L.asr_conv1_7x7s2_wgrad(p(x), p(dy), B, T, Fw, p(out), p(ws), nbytes, st)
            else:
                rc = L.asr_conv1c_7x7s2_wgrad(p(x), p(dy), B, T, Fw, cin, p(out), p(ws), nbytes, st)
    assert rc == N.ASR_OK, '%s returned %d (%s)' % (cr.case_id(case), rc, L.asr_strerror(rc))
    torch.cuda.synchronize()
    bf16 = op in cr.BF16_OUT
    assert guards_intact(buf, torch.bfloat16 if bf16 else torch.float32, cr.POISON_H if bf16 else cr.POISON_F), \
        '%s wrote outside its output' % cr.case_id(case)
    got = dict(out=logical(out) if bf16 else out.cpu().double().numpy(), sums=None)
    if sums is not None:
        assert guards_intact(sums_buf, torch.float64, cr.POISON_F)
        got['sums'] = sums.cpu().numpy()
    return got


def check(case, kinds=('integer', 'gaussian')):
    for kind in kinds:
        inp = cr.integer_inputs(case) if kind == 'integer' else cr.gaussian_inputs(case)
        want = cr.reference(case, inp)
        got = launch(case, inp)
        stats = {}
        bad = cr.judge(case, got, want, kind, stats)
        if stats:
            print('MEASURED %s %s' % (cr.case_id(case), ' '.join('%s %.4g' % kv for kv in sorted(stats.items()))))
        assert not bad, (cr.case_id(case), kind, bad)


def persistent_loops_are_reached(case):
    """the persistent cases must give a workgroup a second item on THIS device"""
    if case['name'] != 'persist' or case['op'] not in ('c32_fwd', 'c32_dgrad'):
        return
    wgs = 2 * torch.cuda.get_device_properties(DEV).multi_processor_count
    items = cr.plan(case['op'], case['shape'])['items']
    assert items > wgs, 'persist: %d items, %d workgroups: no second item, no flipped roles' % (items, wgs)


def params(op):
    sel = [c for c in CASES if c['op'] == op]
    return pytest.mark.parametrize('case', sel, ids=[c['name'] for c in sel])


@params('c32_fwd')
def test_forward(case):
    persistent_loops_are_reached(case)
    check(case)


@params('c32_dgrad')
def test_input_gradient(case):
    persistent_loops_are_reached(case)
    check(case)


@params('c32_wgrad')
def test_weight_gradient(case):
    check(case)


@params('c1_fwd')
def test_first_convolution_forward(case):
    check(case)


@params('c1_wgrad')
def test_first_convolution_weight_gradient(case):
    check(case)


@params('c1c_fwd')
def test_first_convolution_three_channels_forward(case):
    check(case)


@params('c1c_wgrad')
def test_first_convolution_three_channels_weight_gradient(case):
    check(case)


# ---- a width the launchers reject takes the torch path, with its warning ----------------------

@pytest.mark.parametrize('Fw,which,native_node', [
    (30, 'second', 'Conv1BNHardtanhFunctionBackward'),      # conv1 gives W = 12: the forward launcher refuses
    (100, 'first', 'Conv7x7C32FunctionBackward'),           # Fo = 47 > 39: conv1 refuses, W = 47 runs
])
def test_rejected_width_takes_the_torch_path(Fw, which, native_node):
    """the gate of the refused convolution says no, the encoder warns once and goes through torch /
    MIOpen for it (the launcher's ASR_EUNSUPPORTED would be an exception in the middle of the step);
    the other convolution stays native"""
    from att_speech.modules.encoders import DeepSpeech2
    torch.manual_seed(7)
    enc = DeepSpeech2({'features': torch.randn(2, 40, Fw, 1)}, conv_kernel_sizes=[[7, 7], [7, 7]],
                      conv_strides=[[1, 2], [3, 1]], rnn_hidden_size=32, rnn_nb_layers=1,
                      rnn_normalization='none').cuda().train()
    feats = torch.randn(2, 1, 40, Fw, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.warns(UserWarning, match='the %s convolution is not' % which):
        out = enc._conv_forward(feats)
    Fo = (Fw - 7) // 2 + 1
    assert tuple(out.shape) == ((40 + 6 - 7) // 3 + 1, 2, 32 * (Fo - 6))
    out.float().square().sum().backward()
    torch.cuda.synchronize()
    nodes, todo = set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is not None and fn not in nodes:
            nodes.add(fn)
            todo.extend(f for f, _ in fn.next_functions)
    names = {type(n).__name__ for n in nodes}
    refused = 'Conv7x7C32FunctionBackward' if which == 'second' else 'Conv1'
    assert native_node in names and not any(n.startswith(refused) for n in names), names
    for k, prm in enc.conv.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), k


# ---- every width the gates claim runs, and runs exactly ---------------------------------------

def test_every_claimed_width_of_the_second_convolution():
    """B = 2 and the smallest H at which forward, input gradient and weight gradient all have two
    row blocks, at every W native_conv.supported claims: no error code, exact outputs"""
    N = native()
    widths = [W for W in range(7, 65) if N.conv7x7c32_supported(2, 64, W, 3)]
    assert len(widths) == 38
    for W in widths:
        blocks = max(cr.plan('c32_fwd', (2, 64, W, 3))['R'], cr.plan('c32_dgrad', (2, 64, W, 3))['Rq'],
                     cr.plan('c32_wgrad', (2, 64, W, 3))['rows'])
        H = 3 * blocks + 7
        assert N.conv7x7c32_supported(2, H, W, 3)
        for op in ('c32_fwd', 'c32_dgrad', 'c32_wgrad'):
            check(dict(op=op, name='claimed_w%d' % W, shape=(2, H, W, 3)), kinds=('integer',))


@pytest.mark.parametrize('cin', [1, 3])
def test_every_claimed_width_of_the_first_convolution(cin):
    """B = 2 and the smallest T with two row blocks (To = rows + 1), at every F conv1_supported claims"""
    N = native()
    widths = [Fw for Fw in range(7, 201) if N.conv1_supported(Fw, cin)]
    assert len(widths) == (78 if cin == 1 else 40)
    ops, T = (('c1_fwd', 'c1_wgrad'), cr.C1_ROWS + 1 - 6) if cin == 1 else (('c1c_fwd', 'c1c_wgrad'), cr.C1C_ROWS + 1 - 6)
    for Fw in widths:
        for op in ops:
            check(dict(op=op, name='claimed_f%d' % Fw, shape=(2, T, Fw)), kinds=('integer',))
