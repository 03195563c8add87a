"""Bidirectional bias-free GRU layer on the MI355X: dense projections as bf16 GEMMs with fp32
accumulation, the recurrence in the hand-written persistent MFMA kernels of csrc/gru.hip
(include/asr_amd.h: asr_gru_bidir_{fwd,bwd}_bf16).

Replaces torch's nn.GRU behind `BatchRNN.rnn` when the encoder is built with rnn_type=GRU,
keeping the nn.GRU parameter tensors (weight_ih_l0, weight_hh_l0, *_reverse), so state_dict
keys and optimizers are unchanged.  The layout follows native_lstm.py with three gates (r, z, n)
instead of four."""
import torch

from att_speech import _native
from att_speech.modules.encoders.native_lstm import _bmm_f32, _chunks, _mm_f32


class BiGRUFunction(torch.autograd.Function):
    """y[T,B,2,H] = BiGRU(x[T,B,F]; W_ih[2][3H,F], W_hh[2][3H,H]), masked by lens;
    sum_dirs: return y.sum(2) [T,B,H] (BatchRNN's direction merge) so the backward kernel
    reads the one shared gradient."""

    @staticmethod
    def forward(ctx, x, lens_dev, w_ih_f, w_hh_f, w_ih_r, w_hh_r, sum_dirs=False):
        T, B, F = x.shape
        H = w_hh_f.shape[1]
        xb = x.reshape(T * B, F).to(torch.bfloat16)
        ctx.x_bf16 = x.dtype == torch.bfloat16        # then the input gradient is bf16 too
        w_ih = torch.cat([w_ih_f, w_ih_r], 0).to(torch.bfloat16)        # [2*3H, F]
        whh = torch.stack([w_hh_f, w_hh_r], 0).to(torch.bfloat16).contiguous()
        gx = _mm_f32(xb, w_ih.t()).view(T, B, 2, 3 * H)
        y, ybf, gates = _native.gru_bidir_fwd(gx, whh, lens_dev)
        ctx.save_for_backward(xb, lens_dev, w_ih, whh, y, ybf, gates)
        return y.sum(2) if sum_dirs else y

    @staticmethod
    def backward(ctx, dy):
        xb, lens_dev, w_ih, whh, y, ybf, gates = ctx.saved_tensors
        T, B, _, H = y.shape
        F = xb.shape[1]
        whhT = whh.transpose(1, 2).contiguous()                          # [2,H,3H]
        dgx, dhn = _native.gru_bidir_bwd(dy.contiguous(), whhT, lens_dev, gates, y)
        TB = T * B
        dg2 = dgx.view(TB, 6 * H)
        dx = (torch.mm(dg2, w_ih) if ctx.x_bf16 else _mm_f32(dg2, w_ih)).view(T, B, F)
        dw_ih, dw_hh = _weight_gradients(dgx, dhn, xb, ybf, T, B, H, F)
        return dx, None, dw_ih[:3 * H], dw_hh[0], dw_ih[3 * H:], dw_hh[1], None


def _weight_gradients(dgx, dhn, xb, ybf, T, B, H, F):
    """dW_ih [2*3H, F] from (dr, dz, dn) and the layer input; dW_hh[d] [3H, H] from
    (dr, dz, dhn) and h_{t-1} (the forward direction looks one frame back in its zero-padded
    bf16 plane, the reverse one frame ahead).  Chunked library products with fp32
    accumulation, the chunks summed in a fixed order (asr_sum_leading_f32): deterministic."""
    TB = T * B
    g1, g2 = _chunks(TB, 64), _chunks(TB, 32)
    dw_ih = _native.sum_leading(_bmm_f32(dgx.view(g1, TB // g1, 6 * H).transpose(1, 2),
                                         xb.view(g1, TB // g1, F)))
    dgd, dhd = dgx.view(T, B, 2, 3 * H), dhn.view(T, B, 2, H)
    dw_hh = []
    for d in range(2):
        dgh = torch.cat([dgd[:, :, d, :2 * H], dhd[:, :, d]], -1)        # [T,B,3H] (dr, dz, dhn)
        hp = ybf[0, 0:T] if d == 0 else ybf[1, 2:T + 2]
        dw_hh.append(_native.sum_leading(_bmm_f32(dgh.view(g2, TB // g2, 3 * H).transpose(1, 2),
                                                  hp.reshape(g2, TB // g2, H))))
    return dw_ih, dw_hh


def bigru(x, lens, rnn, sum_dirs=False):
    """x [T,B,F] GPU tensor, lens [B] (any int tensor), rnn: nn.GRU(bidirectional,
    bias=False, 1 layer).  Returns per-direction outputs [T,B,2,H], or their sum [T,B,H]
    with sum_dirs."""
    lens_dev = _native.lens_on(lens, x.device)
    return BiGRUFunction.apply(
        x.contiguous(), lens_dev, rnn.weight_ih_l0, rnn.weight_hh_l0,
        rnn.weight_ih_l0_reverse, rnn.weight_hh_l0_reverse, sum_dirs)
