"""asr_conv1_7x7s2_wgrad_bn (csrc/conv.hip): the first convolution's weight gradient with the
backward pass of the BatchNorm + Hardtanh behind it applied on the way in, against the two
kernels it replaces on the same inputs — phase 2 of asr_bn_act_bwd_phase_f32 storing the
gradient of the convolution's output, asr_conv1_7x7s2_wgrad reading it back.  Nothing in the
arithmetic differs, so every comparison is torch.equal."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

LO, HI = 0.0, 20.0

# (B, T, F).  F = 40 -> Fo = 17, the <5, 2> kernel: 7 output rows in one partial chunk; exactly
# one 16-row chunk; a 1-row second chunk and the chunk -> utterance mapping; three chunks per
# utterance; more chunks than some workgroups get.  F = 47 -> Fo = 21, the <8, 3> kernel.
SHAPES = [(1, 1, 40), (1, 10, 40), (3, 11, 40), (2, 40, 40), (5, 37, 40), (2, 40, 47)]
# F = 81 -> Fo = 38, the <16, 6> kernel (Fo 33 .. 39; wider rows do not fit its LDS images):
# its prefetch registers have no room for the z pieces, the width stays on the pair
F_REJECTED = 81


def _inputs(B, T, F, bias, seed=0):
    """gamma = beta = 10 on unit-variance z: y ~ N(10, 10^2), a sixth of the elements below lo,
    a sixth above hi; mean, invstd and the bias differ from channel to channel"""
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(1000 * B + 10 * T + F + seed)
    To, Fo = T + 6, (F - 7) // 2 + 1
    x = torch.randn(B, T, F, generator=g)
    z = torch.randn(B, 32, To, Fo, generator=g)
    dy = torch.randn(B, 32, To, Fo, generator=g)
    mean = 0.05 * torch.randn(32, generator=g)
    invstd = 1.0 + 0.02 * torch.randn(32, generator=g)
    cb = 0.05 * torch.randn(32, generator=g) if bias else None
    nhwc = lambda t: t.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return dict(x=x.to(dev), z=nhwc(z), dy=nhwc(dy), gamma=torch.full((32,), 10.0, device=dev),
                beta=torch.full((32,), 10.0, device=dev), mean=mean.to(dev), invstd=invstd.to(dev),
                cb=None if cb is None else cb.to(dev))


def _mask_shares(d):
    shift = d['mean'] if d['cb'] is None else d['mean'] - d['cb']
    c = lambda v: v.view(1, 32, 1, 1)
    y = (d['z'].float() - c(shift)) * c(d['invstd']) * c(d['gamma']) + c(d['beta'])
    share = lambda m: float(m.float().mean())
    return share(y <= LO), share((y > LO) & (y < HI)), share(y >= HI)


def _pair(d, training, scale_sums):
    """the reference: BatchNorm backward storing dz (phase 1, the sums rescaled the way an
    all-reduce over replicas would, phase 2), then the plain weight gradient"""
    from att_speech import _native

    def sync(sums, n_local):
        if scale_sums:
            sums.mul_(0.5)
            return 2.0 * n_local
        return n_local
    dz, dgamma, dbeta, dcb = _native.bn_act_bwd(
        d['z'], d['gamma'], d['beta'], d['mean'], d['invstd'], training, LO, HI, d['dy'],
        conv_bias=d['cb'], sync=sync if training else None)
    return _native.conv1_wgrad(d['x'], dz), dgamma, dbeta, dcb


def _fused(d, training, scale_sums):
    from att_speech import _native
    ws, dgamma, dbeta, dcb = _native.bn_act_bwd_sums(
        d['z'], d['gamma'], d['beta'], d['mean'], d['invstd'], training, LO, HI, d['dy'],
        conv_bias=d['cb'])
    n = float(d['z'].shape[0] * d['z'].shape[2] * d['z'].shape[3])
    if scale_sums:
        ws[:2 * 32 * 8].view(torch.float64).mul_(0.5)
        n *= 2.0
    dw = _native.conv1_wgrad_bn(d['x'], d['z'], d['dy'], d['cb'], d['gamma'], d['beta'], d['mean'],
                                d['invstd'], training, LO, HI, ws, n)
    return dw, dgamma, dbeta, dcb


def _assert_same(got, want):
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.isfinite(a).all()
            assert torch.equal(a, b)


@pytest.mark.parametrize('B,T,F', SHAPES)
@pytest.mark.parametrize('training,bias,scale_sums', [
    (True, True, False),      # training, with a convolution bias
    (True, False, False),     # without one
    (False, True, False),     # running statistics: k1 = k2 = 0
    (True, True, True),       # sums and count that are not this tensor's own (sync-BN)
])
def test_fused_weight_gradient_equals_the_two_kernels(B, T, F, training, bias, scale_sums):
    from att_speech import _native
    assert _native.conv1_wgrad_bn_supported(F)
    d = _inputs(B, T, F, bias)
    shares = _mask_shares(d)
    print('mask shares (below, inside, above):', shares)
    assert min(shares) >= 0.05
    want = _pair(d, training, scale_sums)
    got = _fused(d, training, scale_sums)
    torch.cuda.synchronize()
    print('max |dW| %.4g, max |dW fused - dW pair| %.4g' % (
        float(want[0].abs().max()), float((got[0] - want[0]).abs().max())))
    assert float(want[0].abs().max()) > 0
    _assert_same(got, want)


def test_rejected_width_keeps_the_pair():
    """Fo = 38: the query says no, the entry point refuses, and the encoder's front-end builds
    the two separate autograd nodes as before"""
    from att_speech import _native
    assert _native.conv1_supported(F_REJECTED, 1)
    assert not _native.conv1_wgrad_bn_supported(F_REJECTED)
    assert not _native.conv1_wgrad_bn_supported(6)
    d = _inputs(1, 3, F_REJECTED, True)
    with pytest.raises(NotImplementedError):
        _fused(d, True, False)
    enc = _encoder(F_REJECTED)
    feats = torch.randn(2, 1, 20, F_REJECTED, generator=torch.Generator().manual_seed(1)).cuda()
    grads, stats, nodes = _front_end(enc, feats)
    assert 'Conv1BNHardtanhFunctionBackward' not in nodes and 'Conv1FunctionBackward' in nodes
    assert all(torch.isfinite(g).all() for g in grads.values())


def _encoder(F):
    from att_speech.modules.encoders import DeepSpeech2
    torch.manual_seed(7)
    sample = {'features': torch.randn(2, 40, F, 1)}
    enc = DeepSpeech2(sample, conv_kernel_sizes=[[7, 7], [7, 7]], conv_strides=[[1, 2], [3, 1]],
                      rnn_hidden_size=32, rnn_nb_layers=1, rnn_normalization='none')
    with torch.no_grad():                    # parameters a BatchNorm backward can tell apart
        for i in (1, 4):
            bn = enc.conv[i].batch_norm
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    return enc.cuda().train()


def _front_end(enc, feats):
    """conv1 -> BN -> conv2 -> BN of a copy of `enc`: parameter gradients, running statistics
    and the names of the autograd nodes behind the output"""
    enc = copy.deepcopy(enc)
    out = enc._conv_forward(feats)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).to(out.device)
    (out.float() * w).sum().backward()
    torch.cuda.synchronize()
    nodes, todo = set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is not None and fn not in nodes:
            nodes.add(fn)
            todo.extend(f for f, _ in fn.next_functions)
    grads = {k: p.grad for k, p in enc.conv.named_parameters()}
    stats = {k: b.clone() for k, b in enc.conv.named_buffers()}
    return grads, stats, {type(n).__name__ for n in nodes}


def test_encoder_front_end_equals_the_unfused_pair(monkeypatch):
    from att_speech.modules.encoders import native_conv
    enc = _encoder(40)
    feats = torch.randn(2, 1, 40, 40, generator=torch.Generator().manual_seed(1)).cuda()
    g1, s1, n1 = _front_end(enc, feats)
    assert 'Conv1BNHardtanhFunctionBackward' in n1
    monkeypatch.setattr(native_conv, 'conv1_bn_supported', lambda conv, features: False)
    g0, s0, n0 = _front_end(enc, feats)
    assert 'Conv1BNHardtanhFunctionBackward' not in n0 and 'Conv1FunctionBackward' in n0
    assert set(g1) == set(g0) and set(s1) == set(s0) and len(g1) == 8
    for k in g0:
        assert g0[k] is not None and torch.isfinite(g0[k]).all(), k
        # (a convolution bias in front of a training BatchNorm has no gradient: exact zeros)
        assert float(g0[k].abs().max()) > 0 or k in ('0.bias', '3.bias'), k
        assert torch.equal(g1[k], g0[k]), k
    for k in s0:
        assert torch.equal(s1[k], s0[k]), k
