"""The encoder's 32 -> 32 channel 7x7 convolution (reference deep_speech_2.py:60-73,
Conv2d(32, 32, (7, 7), stride (3, 1))) as one autograd function over the hand-written MFMA
kernels of csrc/conv.hip (include/asr_amd.h: asr_conv7x7c32_{fwd,bwd_data,wgrad}_bf16):
channels-last bf16 activations, fp32 accumulation, fp32 weight gradient, bias-free (the bias
lives in the fused BatchNorm kernels).  The module keeps its nn.Conv2d parameters (state_dict
keys `conv.3.{weight,bias}` unchanged)."""
import torch

from att_speech import _native
from att_speech.modules.encoders import native_bn


def supported(conv, x):
    """the shapes csrc/conv.hip is built for — as its launchers themselves report them
    (asr_conv7x7c32_supported: forward, input gradient and weight gradient all take B, H, W);
    anything else stays on torch / MIOpen"""
    return (x.is_cuda and isinstance(conv, torch.nn.Conv2d) and conv.in_channels == 32
            and conv.out_channels == 32 and tuple(conv.kernel_size) == (7, 7)
            and tuple(conv.stride) == (3, 1) and tuple(conv.padding) == (0, 0)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and x.dim() == 4 and x.size(1) == 32
            and _native.conv7x7c32_supported(x.size(0), x.size(2), x.size(3), conv.stride[0]))


class Conv7x7C32Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(x, weight)
        y, sums = _native.conv7x7c32_fwd(x, weight.detach(), 3, want_sums=True)
        ctx.mark_non_differentiable(sums)
        return y, sums

    @staticmethod
    def backward(ctx, dy, _dsums):
        x, weight = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _native.conv7x7c32_bwd_data(dy, weight.detach(), x.size(2), x.size(3), 3)
        if ctx.needs_input_grad[1]:
            dw = _native.conv7x7c32_wgrad(x, dy, 3)
        return dx, dw


def first_supported(conv, x):
    """Conv2d(cin, 32, (7, 7), stride (1, 2), padding (6, 0)) on [B, cin, T, F] features: one
    channel (the synthetic 40-dim benchmark features), or the WSJ recipes' three (81 mel bins:
    static, delta, delta-delta) with an even output width"""
    return (x.is_cuda and isinstance(conv, torch.nn.Conv2d) and conv.in_channels in (1, 3)
            and conv.out_channels == 32 and tuple(conv.kernel_size) == (7, 7)
            and tuple(conv.stride) == (1, 2) and tuple(conv.padding) == (6, 0)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and x.dim() == 4 and x.size(1) == conv.in_channels
            and _native.conv1_supported(x.size(3), conv.in_channels)
            and not x.requires_grad)        # the kernel pair computes no feature gradient


class Conv1Function(torch.autograd.Function):
    """features [B, T, F] or [B, T, F, cin] f32 -> [B, 32, T + 6, Fo] channels-last bf16; the
    features need no gradient, the weight gradient is asr_conv1{,c}_7x7s2_wgrad"""

    @staticmethod
    def forward(ctx, x, weight):
        x = x.float().contiguous()
        ctx.save_for_backward(x, weight)
        y, sums = _native.conv1_fwd(x, weight.detach(), want_sums=True)
        ctx.mark_non_differentiable(sums)
        return y, sums

    @staticmethod
    def backward(ctx, dy, _dsums):
        x, weight = ctx.saved_tensors
        return None, (_native.conv1_wgrad(x, dy) if ctx.needs_input_grad[1] else None)


class Conv1BNHardtanhFunction(torch.autograd.Function):
    """one-channel features [B, T, F] f32 -> Hardtanh(BatchNorm2d(conv1(features) + bias)),
    [B, 32, T + 6, Fo] channels-last bf16.  Forward: Conv1Function's and BNHardtanhFunction's
    two kernels.  Backward: the BatchNorm's sums pass, then asr_conv1_7x7s2_wgrad_bn, which
    applies the BatchNorm backward to the gradient on its way into the weight-gradient product:
    the gradient of the convolution's output — a tensor as large as the output, with this one
    reader since the features need no gradient — is never stored."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, conv_bias, running_mean, running_var, training,
                momentum, eps, lo, hi, sync):
        x = x.float().contiguous()
        z, sums = _native.conv1_fwd(x, weight.detach(), want_sums=True)
        sync_counts = None
        if sync:
            sums, sync_counts = native_bn.synced_chan_sums(z, sums)
        out, mean, invstd = _native.bn_act_fwd(
            z, gamma.detach(), beta.detach(), running_mean, running_var, training, momentum, eps,
            lo, hi, out_bf16=True, conv_bias=None if conv_bias is None else conv_bias.detach(),
            chan_sums=sums if training else None)
        native_bn.correct_running_var(running_var, invstd, momentum, eps, sync_counts)
        ctx.has_cb = conv_bias is not None
        ctx.save_for_backward(x, weight, z, gamma, beta, mean, invstd,
                              conv_bias if conv_bias is not None else gamma)
        ctx.cfg = (training, lo, hi)
        ctx.sync = training and native_bn._sync_active()
        return out

    @staticmethod
    def backward(ctx, dy):
        x, weight, z, gamma, beta, mean, invstd, cb = ctx.saved_tensors
        training, lo, hi = ctx.cfg
        cb = cb.detach() if ctx.has_cb else None
        sync = native_bn._allreduce_sums if ctx.sync else None
        if dy.dtype != torch.bfloat16:      # (a gradient the fused kernel does not read: the pair)
            dz, dgamma, dbeta, dcb = _native.bn_act_bwd(
                z, gamma.detach(), beta.detach(), mean, invstd, training, lo, hi, dy,
                conv_bias=cb, sync=sync)
            dw = _native.conv1_wgrad(x, dz) if ctx.needs_input_grad[1] else None
            return (None, dw, dgamma, dbeta, dcb) + (None,) * 8
        ws, dgamma, dbeta, dcb = _native.bn_act_bwd_sums(
            z, gamma.detach(), beta.detach(), mean, invstd, training, lo, hi, dy, conv_bias=cb)
        n_total = float(z.shape[0]) * z.shape[2] * z.shape[3]
        if sync is not None:
            n_total = sync(ws[:2 * z.shape[1] * 8].view(torch.float64), n_total)
        dw = None
        if ctx.needs_input_grad[1]:
            dw = _native.conv1_wgrad_bn(x, z, dy, cb, gamma.detach(), beta.detach(), mean, invstd,
                                        training, lo, hi, ws, n_total)
        return (None, dw, dgamma, dbeta, dcb) + (None,) * 8


def conv1_bn_supported(conv, features):
    """first_supported shapes whose weight gradient can apply the BatchNorm backward itself"""
    return conv.in_channels == 1 and _native.conv1_wgrad_bn_supported(features.size(3))


def conv1_bn_hardtanh(features, conv, bn, act):
    """features logical [B, 1, T, F] -> Hardtanh(bn(conv(features))) as channels-last bf16:
    conv1 and native_bn.bn_hardtanh(out_bf16=True, conv_bias=conv.bias) as one autograd node"""
    use_batch_stats, momentum, rm, rv = native_bn.batch_stats_config(bn)
    sync = use_batch_stats and bn.training and native_bn._sync_active()
    return Conv1BNHardtanhFunction.apply(
        features[:, 0], conv.weight, bn.weight, bn.bias, conv.bias, rm, rv, use_batch_stats,
        momentum, bn.eps, float(act.min_val), float(act.max_val), sync)


def conv1(features, conv):
    """features logical [B, cin, T, F] (any strides; the reference's [B, T, F, cin] batches
    arrive as a permuted view, deep_speech_2.py:127) -> (conv(features) without the bias, its
    channel sums [2, 32] f64 for the following BatchNorm)"""
    if features.size(1) == 1:
        return Conv1Function.apply(features[:, 0], conv.weight)
    return Conv1Function.apply(features.permute(0, 2, 3, 1), conv.weight)


def conv7x7c32(x, conv):
    """(y = conv(x) without the bias: logical [B, 32, Ho, Wo] bf16, channels-last memory;
    channel sums [2, 32] f64 of y for the following BatchNorm)"""
    return Conv7x7C32Function.apply(x, conv.weight)
