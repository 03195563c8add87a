"""att_speech.modules.tcn — the stage-2 decoder of the reference
(att_speech/modules/tcn.py): a causal dilated-convolution language model over
the label history (`TCN` of `TemporalBlock`s, :46-116), a location-aware
`LocalAttention` (:119-230) and `AttentionDecoderTCN` (:233-585) with the
teacher-forced training `forward` (:357-440) and the step-wise beam `decode`
(:442-585; plain BeamSearch, or with `lm_file` the LM-fused BeamSearchLM /
RescoreSearchLM / GraphSearch over an att_speech.lm_fst.LmFst), plus
`score_sentences`, the teacher-forced rescoring pass of the reference's
egs/wsj/local/lattice_search scripts.

Kept from the reference: class names, constructor keywords, the returned dicts
and the checkpoint keys (`tcn.network.<i>.net.conv<j>.{bias,weight_g,weight_v}`,
`attn.{encoded_to_hidden,hidden_to_score,lm_to_kernel,lm_to_global,
encoded_to_init_weights}.*`, `combined_to_output.{0,3}.*`, ...).  Organisation and
arithmetic layout are this build's:

* a causal convolution pads on the left only (the reference pads both sides and
  chops the right end off again);
* time runs along the LAST axis of every attention tensor (`[hyp, T']` rows):
  the location filter is one batched product over sliding windows of the previous
  alignment, the softmax and the context reduce over contiguous rows;
* the training targets (one-hot, smoothed along time, renormalised) and the
  accuracy are built without Python loops over the batch.
"""
from __future__ import absolute_import, division, print_function

import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from att_speech import fst_utils
from att_speech.lm_fst import LmFst
from att_speech.modules import beam_search as bs
from att_speech.modules.beam_search import (BeamSearch, BeamSearchLM, GraphSearch,
                                             RescoreSearchLM)

_MASKED = -1e5          # additive score of a padded encoder frame


class _CausalConv1d(nn.Conv1d):
    """Dilated 1-D convolution whose output at time t sees inputs <= t."""

    def __init__(self, channels_in, channels_out, taps, dilation):
        super(_CausalConv1d, self).__init__(channels_in, channels_out, taps, dilation=dilation)
        self.history = (taps - 1) * dilation

    def forward(self, x):                       # [batch, channels, time]
        return F.conv1d(F.pad(x, (self.history, 0)), self.weight, self.bias,
                        dilation=self.dilation)


class TemporalBlock(nn.Module):
    """`n_layers` weight-normalised causal convolutions, each followed by ReLU and
    channel dropout, plus a residual connection (1x1 convolution when the channel
    count changes).  Parameters live under `net.conv<j>` / `downsample`."""

    def __init__(self, n_inputs, n_outputs, kernel_size, stride, dilation,
                 padding, dropout=0.2, n_layers=2):
        super(TemporalBlock, self).__init__()
        if stride != 1 or padding != (kernel_size - 1) * dilation:
            raise ValueError("TemporalBlock: only the causal stride-1 form the TCN builds")
        self.net = nn.ModuleDict()
        for j in range(n_layers):
            conv = _CausalConv1d(n_outputs if j else n_inputs, n_outputs, kernel_size, dilation)
            # weight_g / weight_v parametrisation; like the reference, the N(0, 0.01)
            # draw it makes afterwards lands in the derived `.weight` and is overwritten
            # by the next forward, so the effective initialisation is Conv1d's default
            self.net['conv%d' % j] = torch.nn.utils.weight_norm(conv)
        self.channel_dropout = dropout
        self.downsample = None
        if n_inputs != n_outputs:
            self.downsample = nn.Conv1d(n_inputs, n_outputs, 1)
            nn.init.normal_(self.downsample.weight, 0.0, 0.01)

    def forward(self, x):                       # [batch, channels, time]
        y = x
        for conv in self.net.values():
            y = F.dropout1d(torch.relu(conv(y)), self.channel_dropout, self.training)
        shortcut = x if self.downsample is None else self.downsample(x)
        return torch.relu(y + shortcut)


class TCN(nn.Module):
    """Stack of TemporalBlocks, one per entry of `dilation_sizes`."""

    def __init__(self, num_inputs, num_channels, dilation_sizes, kernel_size=2,
                 dropout=0.2, layers_per_block=2):
        super(TCN, self).__init__()
        if len(num_channels) != len(dilation_sizes):
            raise ValueError('num_channels and dilations_sizes lengths '
                             'must be equal (number of blocks)')
        # label history the decoder feeds per step (reference :93)
        self.eff_history = 1 + (kernel_size - 1) * sum(dilation_sizes)
        widths = [num_inputs] + list(num_channels)
        self.network = nn.Sequential(*[
            TemporalBlock(widths[i], widths[i + 1], kernel_size, stride=1, dilation=d,
                          padding=(kernel_size - 1) * d, dropout=dropout,
                          n_layers=layers_per_block)
            for i, d in enumerate(dilation_sizes)])

    def forward(self, x):                       # [time, batch, channels] in and out
        return self.network(x.permute(1, 2, 0)).permute(2, 0, 1)

    def last_step_plan(self, steps):
        """Operands for `last_step` over a window of `steps` frames: per block the frames its
        output is needed at, and per convolution (weight [taps*Cin, Cout] with the
        weight-norm already applied, bias, tap source indices).  Only what the LAST output
        frame depends on is computed — 18 of the 28 frame x layer pairs for the tcn.yaml
        stack — as dense products over all hypotheses."""
        blocks = list(self.network)
        need = [None] * (len(blocks) + 1)
        need[-1] = [steps - 1]
        plans = [None] * len(blocks)
        for bi in range(len(blocks) - 1, -1, -1):
            convs = list(blocks[bi].net.values())
            outs, cur = [], need[bi + 1]
            for conv in reversed(convs):
                taps, dil = conv.kernel_size[0], conv.dilation[0]
                src = sorted({t - (taps - 1 - j) * dil for t in cur for j in range(taps)} - set(
                    range(-steps * taps * dil, 0)))
                outs.append((conv, cur, src))
                cur = src
            need[bi] = sorted(set(cur) | set(need[bi + 1]))          # + the residual input
            layers, avail = [], need[bi]
            for conv, out_pos, _ in reversed(outs):
                taps, dil = conv.kernel_size[0], conv.dilation[0]
                w = torch._weight_norm(conv.weight_v, conv.weight_g, 0).detach()
                # row index into [zero frame] + available frames, per (output frame, tap)
                idx = [[(avail.index(t - (taps - 1 - j) * dil) + 1) if t - (taps - 1 - j) * dil >= 0 else 0
                        for j in range(taps)] for t in out_pos]
                layers.append((w.permute(2, 1, 0).reshape(-1, w.size(0)).contiguous(),
                               conv.bias.detach(), torch.tensor(idx, device=w.device)))
                avail = out_pos
            res_idx = torch.tensor([need[bi].index(t) for t in need[bi + 1]], device=w.device)
            plans[bi] = (layers, res_idx, blocks[bi].downsample)
        return need[0], plans

    @staticmethod
    def last_step(x, plan):
        """x [steps, hyp, C] -> LM state of the last frame [hyp, C] (eval mode)."""
        first_need, plans = plan
        cur = x[first_need] if len(first_need) != x.size(0) else x        # [n, hyp, C]
        for layers, res_idx, downsample in plans:
            y = cur
            for weight, bias, idx in layers:
                padded = torch.cat((torch.zeros_like(y[:1]), y))            # frame 0 = zeros
                cols = padded[idx]                                          # [out, taps, hyp, C]
                n_out, taps, hyps, ch = cols.shape
                cols = cols.permute(0, 2, 1, 3).reshape(n_out * hyps, taps * ch)
                y = torch.relu(torch.addmm(bias, cols, weight)).view(n_out, hyps, -1)
            shortcut = cur[res_idx]
            if downsample is not None:
                shortcut = downsample(shortcut.permute(1, 2, 0)).permute(2, 0, 1)
            cur = torch.relu(y + shortcut)
        return cur[-1]


class LocalAttention(nn.Module):
    """Location-aware additive attention: the score of encoder frame t for a
    hypothesis is  w . tanh(E_t + (a_prev * k)(t) + g)  with E the projected encoder
    output, k a per-hypothesis filter predicted from the LM state that is slid
    causally over the previous alignment a_prev, and g a global LM term."""

    def __init__(self, encoded_size, lm_state_size, hidden_size, kernel_size=32,
                 temperature=1.0, force_forward=None, learnable_init=True, **kwargs):
        super(LocalAttention, self).__init__(**kwargs)
        self.encoded_size, self.kernel_size = encoded_size, kernel_size
        self.temperature, self.force_forward = temperature, force_forward
        self.learnable_init = learnable_init
        self.encoded_to_hidden = nn.Linear(encoded_size, hidden_size)
        self.hidden_to_score = nn.Linear(hidden_size, 1)
        nn.init.zeros_(self.hidden_to_score.weight)     # start from a uniform alignment
        self.lm_to_kernel = nn.Linear(lm_state_size, kernel_size * hidden_size)
        self.lm_to_global = nn.Linear(lm_state_size, hidden_size)
        self.encoded_to_init_weights = nn.Linear(encoded_size, 1)

    @staticmethod
    def _padding_scores(lens, steps, device):
        """[T', B]: 0 on frames of the utterance, -1e5 behind its end."""
        lens = torch.as_tensor(lens).to(device).long()
        behind = torch.arange(steps, device=device)[:, None] >= lens[None, :]
        return behind.float() * _MASKED

    def init_attention(self, encoded, encoded_lens):
        """encoded [T', B, E] -> ((projected encoder, padding scores), alignment [T', B])"""
        pad = self._padding_scores(encoded_lens, encoded.size(0), encoded.device)
        if self.learnable_init:
            first = F.softmax(self.encoded_to_init_weights(encoded).squeeze(2) + pad, 0)
        else:                                   # all mass on the first frame
            first = torch.zeros_like(pad)
            first[0] = 1.0
        return (self.encoded_to_hidden(encoded), pad), first

    def recompute_forward_mask(self, prev_rows, pad):
        """`force_forward = (lo, hi)`: frames outside [peak+lo, peak+hi) of the previous
        alignment are masked, unless that alignment is diffuse (peak < 0.1).
        prev_rows [hyp, T'], pad [T', hyp]."""
        peak, where = prev_rows.max(1)
        t = torch.arange(pad.size(0), device=pad.device)[:, None]
        lo, hi = where + self.force_forward[0], where + self.force_forward[1]
        outside = ((t < lo[None, :]) | (t >= hi[None, :])) & (peak >= 0.1)[None, :]
        return pad + outside.to(pad.dtype) * _MASKED

    def scores(self, att_state, lm_state, prev_att_weights):
        """Masked, temperature-scaled scores as rows [hyp, T']."""
        projected, pad = att_state                               # [T', hyp, A], [T', hyp]
        steps, hyps, width = projected.shape
        prev_rows = prev_att_weights.t()                         # [hyp, T']
        taps = self.kernel_size
        # (a_prev * k)(t) = sum_j a_prev[t - (taps-1) + j] k[j]: a batched product over
        # sliding windows of the left-padded previous alignment
        windows = F.pad(prev_rows, (taps - 1, 0)).unfold(1, taps, 1)            # [hyp, T', taps]
        filters = self.lm_to_kernel(lm_state).view(hyps, width, taps)
        moved = torch.bmm(windows, filters.transpose(1, 2))                      # [hyp, T', A]
        hidden = projected.transpose(0, 1) + moved + self.lm_to_global(lm_state)[:, None, :]
        energy = self.hidden_to_score(torch.tanh(hidden)).squeeze(2) * self.temperature
        if self.force_forward:
            pad = self.recompute_forward_mask(prev_rows, pad)
        return energy + pad.t()

    def forward(self, att_state, lm_state, prev_att_weights):
        """lm_state [hyp, H], prev_att_weights [T', hyp] -> (att_state, alignment [T', hyp])"""
        rows = F.softmax(self.scores(att_state, lm_state, prev_att_weights), 1)
        return att_state, rows.t()


_SCAN_MAX_FRAMES = 4096     # asr_tcn_attention_scan_*_f32: longest encoder sequence
_SCAN_MAX_WIDTH = 256       # ... and widest attention
_STEP_MAX_FRAMES = 8160     # asr_tcn_attention_step_f32: two alignment rows in 64 KiB of LDS


class _AttentionScan(torch.autograd.Function):
    """The whole training recurrence of LocalAttention over the label positions as one
    autograd node: asr_tcn_attention_scan_fwd_f32 forward, asr_tcn_attention_scan_bwd_f32
    backward (h recomputed, only the alignments saved).
    eproj [T', B, A], filt [L, B, A*K], glob [L, B, A], a0 [T', B], w_score [A],
    b_score [1] -> alignments [L, B, T']."""

    @staticmethod
    def forward(ctx, eproj, filt, glob, a0, w_score, b_score, lens, temperature):
        from att_speech import _native
        eproj, filt, glob = eproj.contiguous(), filt.contiguous(), glob.contiguous()
        a0, w_score = a0.contiguous(), w_score.contiguous()
        att = _native.tcn_attention_scan_fwd(eproj, filt, glob, a0, w_score, b_score, lens,
                                             temperature)
        ctx.save_for_backward(eproj, filt, glob, a0, w_score, lens, att)
        ctx.temperature = temperature
        return att

    @staticmethod
    def backward(ctx, d_att):
        from att_speech import _native
        eproj, filt, glob, a0, w_score, lens, att = ctx.saved_tensors
        d_eproj, d_filt, d_glob, d_a0, d_wb = _native.tcn_attention_scan_bwd(
            eproj, filt, glob, a0, w_score, lens, ctx.temperature, att, d_att.contiguous())
        A = w_score.numel()
        d_wb = d_wb.sum(0)
        return (d_eproj, d_filt, d_glob, d_a0, d_wb[:A], d_wb[A:], None, None)


_SMOOTHING_TAPS = (0.005, 0.02, 0.95, 0.02, 0.005)      # along the label axis (:411-414)

# one warning per process and key (`_native._WARNED`) when a device path gives a call up
_GAVE_UP_WARNINGS = {
    'graph_store': 'the node store of the device graph search would take %d bytes, above its '
                   'budget of %d: decoding this call with the host GraphSearch, one utterance '
                   'at a time',
    'lm_bag_overflow': 'an LM bag of the device beam search asked for at least %d states, above '
                       'its cap of %d: decoding this call with the host BeamSearchLM, one utterance at a time',
    'forced_lm_bag_overflow': 'an LM bag of the device forced scorer asked for at least %d '
                              'states, above its cap of %d: scoring this call with the host '
                              'loop, one sentence at a time'}


class _DeviceStepper(object):
    """The label step of AttentionDecoderTCN on the MI355X, the one place both device paths
    (`_decode_native`, `_score_sentences_native`) take it from.  Built once per call: the
    per-utterance operands (the reference repeats them per hypothesis, :449-456), the
    last-frame plan of the TCN and the filter / global weights as one matrix.  `step` is the LM
    state of the last frame as dense products (TCN.last_step), ONE launch for the local
    attention + context (asr_tcn_attention_step_f32, or asr_tcn_attention_step_win_f32 under a
    force_forward window) and the output MLP; `roll` moves the label history on.  Nothing
    here reads back from the device after the constructor."""

    def __init__(self, decoder, encoded, lens_dev):
        attn, tcn = decoder.attn, decoder.tcn
        self.decoder, self.lens = decoder, lens_dev
        (eproj, _), self.first = attn.init_attention(encoded, lens_dev)   # first: [T, B]
        self.eproj, self.enc = eproj.contiguous(), encoded.contiguous()
        self.plan = tcn.last_step_plan(tcn.eff_history)
        self.w_att = torch.cat((attn.lm_to_kernel.weight, attn.lm_to_global.weight)).detach()
        self.b_att = torch.cat((attn.lm_to_kernel.bias, attn.lm_to_global.bias)).detach()
        self.n_filt = attn.lm_to_kernel.out_features
        self.w_score = attn.hidden_to_score.weight.detach().reshape(-1).contiguous()
        self.b_score = float(attn.hidden_to_score.bias)
        self.window = tuple(attn.force_forward) if attn.force_forward else None

    def empty_history(self, rows):
        tcn = self.decoder.tcn
        return self.enc.new_zeros(tcn.eff_history, rows, self.decoder.tcn_hidden_size)

    def step(self, history, att_prev, parent, group):
        """history [eff_history, rows, D]; att_prev [rows', T] with row r of the output continuing
        row parent[r] of it (None: its own row); `group` rows per utterance -> (logits [rows, C],
        alignment [rows, T])."""
        from att_speech import _native
        n_filt = self.n_filt
        lm_state = TCN.last_step(history, self.plan)
        fg = torch.addmm(self.b_att, lm_state, self.w_att.t())
        att, context = _native.tcn_attention_step(
            self.eproj, self.enc, self.lens, fg[:, :n_filt].contiguous(), fg[:, n_filt:].contiguous(),
            self.w_score, self.b_score, self.decoder.attn.temperature, att_prev, parent, group,
            window=self.window)
        return self.decoder._step_output(lm_state, context), att

    def roll(self, history, parent, labels):
        """the history of the rows that continue rows `parent` with `labels`"""
        return torch.cat((history[1:].index_select(1, parent.long()),
                          self.decoder.embedding(labels.long())[None]))


class AttentionDecoderTCN(nn.Module):
    def __init__(self, sample_batch, num_classes, tcn_hidden_size, att_hidden_size,
                 dropout_p, learnable_initial_attention=True, label_smoothing=True,
                 kernel_size=3, dilation_sizes=[1, 2, 4], coverage_tau=0.5,
                 coverage_weight=0, beam_size=1, length_normalization=0.0,
                 att_force_forward=None, vocabulary=None, branching_threshold=0.0,
                 lm_file=None, lm_weight=1.0, attention_temperature=1.0,
                 tcn_layers_per_block=2, min_attention_pos=0.5, keep_eos_score=False,
                 use_graph_search=False, graph_search_history_len=-1,
                 graph_search_merge_threshold=0.8, **kwargs):
        super(AttentionDecoderTCN, self).__init__(**kwargs)
        # search options
        self.beam_size, self.length_normalization = beam_size, length_normalization
        self.branching_threshold = branching_threshold
        self.coverage_tau, self.coverage_weight = coverage_tau, coverage_weight
        self.min_attention_pos, self.keep_eos_score = min_attention_pos, keep_eos_score
        self.use_graph_search = use_graph_search
        self.graph_search_history_len = graph_search_history_len
        self.graph_search_merge_threshold = graph_search_merge_threshold
        self.lm_weight, self.rescore = lm_weight, None
        self.TRANSCRIPTION_LEN_GUARD = 250
        # sizes; the class inventory gets an end-of-sequence symbol behind the last class
        self.encoded_size = sample_batch["features"].size(2)
        self.tcn_hidden_size, self.att_hidden_size = tcn_hidden_size, att_hidden_size
        self.EOS, self.num_classes = num_classes, num_classes + 1
        self.vocabulary, self.label_smoothing = vocabulary, label_smoothing
        # modules (attribute names are checkpoint keys)
        self.embedding = nn.Embedding(self.num_classes, tcn_hidden_size)
        self.dropout = nn.Dropout(dropout_p)
        self.attn = LocalAttention(self.encoded_size, tcn_hidden_size, att_hidden_size,
                                   temperature=attention_temperature,
                                   learnable_init=learnable_initial_attention,
                                   force_forward=att_force_forward)
        self.tcn = TCN(tcn_hidden_size, [tcn_hidden_size] * len(dilation_sizes),
                       dilation_sizes=dilation_sizes, kernel_size=kernel_size,
                       dropout=dropout_p, layers_per_block=tcn_layers_per_block)
        width = 256
        self.combined_to_output = nn.Sequential(
            nn.Linear(tcn_hidden_size + self.encoded_size, width), nn.ReLU(), nn.Dropout(dropout_p),
            nn.Linear(width, width), nn.ReLU(), nn.Dropout(dropout_p))
        self.output_to_logits = nn.Linear(width, self.num_classes)
        # language model for the fused searches (the reference reads a pywrapfst.Fst, :293-300)
        self.lm = None
        if lm_file:
            assert vocabulary is not None
            self.lm = lm_file if isinstance(lm_file, LmFst) else LmFst.read(lm_file)
        self.alphabet_mapping = self.create_alphabet_mapping()

    def create_alphabet_mapping(self):
        """LM input label of every model class (:306-327): by symbol name, the space as
        '<spc>'; classes the LM does not know — and EOS — also map to '<spc>'."""
        if self.lm is None:
            return None
        label_of = {sym: lab for lab, sym in self.lm.input_symbols()}
        names = ['<spc>' if s == ' ' else s for s in list(self.vocabulary) + ['<eos>']]
        return [label_of.get(name, label_of['<spc>']) for name in names]

    def hash_dec(self, decoded):
        """Merge key of GraphSearch (:335-345): the last `history` labels, left-filled with -1."""
        span = self._graph_span()
        if span == 0:
            return 0
        tail = decoded[-span:].tolist()
        return hash(tuple([-1] * (span - len(tail)) + tail))

    # ---------------------------------------------------------------- training
    def _step_output(self, lm_state, context):
        return self.output_to_logits(self.combined_to_output(torch.cat((lm_state, context), -1)))

    def _smoothed_targets(self, labels):
        """labels [B, L] -> per-position target distributions [B, L, classes]: one-hot,
        optionally smeared over NEIGHBOURING POSITIONS with the 5-tap kernel, renormalised,
        class 0 (padding) removed afterwards (:404-424)."""
        onehot = F.one_hot(labels, self.num_classes).to(torch.float32)        # [B, L, C]
        if self.label_smoothing:
            B, L, C = onehot.shape
            taps = onehot.new_tensor(_SMOOTHING_TAPS).view(1, 1, -1)
            along_time = onehot.transpose(1, 2).reshape(B * C, 1, L)
            onehot = F.conv1d(along_time, taps, padding=len(_SMOOTHING_TAPS) // 2) \
                .view(B, C, L).transpose(1, 2)
        dist = onehot / onehot.sum(2, keepdim=True)
        dist[:, :, 0] = 0
        return dist

    def _native_train_ok(self, encoded):
        """The training recurrence through asr_tcn_attention_scan_*_f32 (read per call;
        ASR_TCN_TRAIN_NATIVE=0 keeps the per-position loop)."""
        if os.environ.get('ASR_TCN_TRAIN_NATIVE', '1') == '0':
            return False
        attn = self.attn
        return (encoded.is_cuda and encoded.dtype == torch.float32
                and attn.kernel_size == 32 and not attn.force_forward
                and 1 <= encoded.size(0) <= _SCAN_MAX_FRAMES
                and 1 <= self.att_hidden_size <= _SCAN_MAX_WIDTH)

    def _forward_scan(self, encoded, encoded_lens, lm_states, eproj, first):
        """All L positions at once: the filter / global LM terms as one product each, the
        alignment recurrence as ONE autograd node (_AttentionScan), every context as one
        batched product and the output MLP once over [B, L, .] -> (alignments [L, B, T'],
        logits [B, L, C]).  In training mode the MLP's
        dropout masks are drawn in that one call (same distribution, another RNG stream)."""
        attn = self.attn
        lens = torch.as_tensor(encoded_lens).to(encoded.device, torch.int32)
        filt = attn.lm_to_kernel(lm_states)                                    # [L, B, A*K]
        glob = attn.lm_to_global(lm_states)                                    # [L, B, A]
        att = _AttentionScan.apply(eproj, filt, glob, first,
                                   attn.hidden_to_score.weight.reshape(-1),
                                   attn.hidden_to_score.bias, lens, attn.temperature)
        contexts = torch.bmm(att.transpose(0, 1), encoded.transpose(0, 1))     # [B, L, E]
        logits = self._step_output(lm_states.transpose(0, 1), contexts)        # [B, L, C]
        return att, logits

    def forward(self, encoded, encoded_lens, texts, text_lens,
                return_att_weights=False, **kwargs):
        """Teacher-forced loss (:357-440): the TCN reads <start> + labels, every label
        position attends from the previous position's alignment; cross-entropy against
        the smoothed targets over labels + EOS."""
        dev = encoded.device
        B, L = texts.size(0), texts.size(1) + 1
        labels = torch.zeros(B, L, dtype=torch.long)
        labels[:, :L - 1] = texts.cpu().long()
        labels[torch.arange(B), torch.as_tensor(text_lens).long()] = self.EOS
        labels = labels.to(dev)
        history = self.embedding(labels.t())                                   # [L, B, D]
        lm_states = self.tcn(torch.cat((torch.zeros_like(history[:1]), history[:-1])))
        att_state, alignment = self.attn.init_attention(encoded, encoded_lens)
        enc_rows = encoded.transpose(0, 1)                                     # [B, T', E]
        if self._native_train_ok(encoded):
            att, logits = self._forward_scan(encoded, encoded_lens, lm_states, att_state[0],
                                             alignment)
            alignments = [a.t() for a in att.unbind(0)] if return_att_weights else None
        else:
            alignments, step_logits = [], []
            for lm_state in lm_states:
                att_state, alignment = self.attn(att_state, lm_state, alignment)
                alignments.append(alignment)
                context = torch.bmm(alignment.t().unsqueeze(1), enc_rows).squeeze(1)
                step_logits.append(self._step_output(lm_state, context))
            logits = torch.stack(step_logits, 1)                               # [B, L, C]
        targets = self._smoothed_targets(labels)
        per_position = -(F.log_softmax(logits, 2) * targets).sum(2)
        loss = per_position.mean() / targets.sum(2).mean()
        # accuracy over non-padding positions
        real = labels != 0
        hits = (logits.argmax(2) == labels) & real
        acc = hits.double().sum() / real.double().sum()
        ret = {'loss': loss, 'acc': acc, 'logits': logits}
        if return_att_weights:
            ret['attweights'] = alignments
        return ret

    # ---------------------------------------------------------------- decoding
    def enc_initial_state(self, encoded, encoded_lens, beam_size, batch_size):
        """Search state for `batch_size * beam_size` hypotheses (hypotheses of one
        utterance adjacent): zero label history, the encoder output and its initial
        alignment repeated per beam entry (:442-463)."""
        hyps = batch_size * beam_size
        per_hyp = encoded.repeat_interleave(beam_size, dim=1)
        lens = torch.as_tensor(encoded_lens).repeat_interleave(self.beam_size)
        att_state, alignment = self.attn.init_attention(per_hyp, lens)
        history = encoded.new_zeros(self.tcn.eff_history, hyps, self.tcn_hidden_size)
        return {'inputs': history, 'encoded': per_hyp, 'att_state': att_state,
                'att_weights': alignment}

    def enc_step(self, inputs, encoded, att_state, att_weights):
        """One label step for every live hypothesis (:465-474): LM state from the last
        `eff_history` embeddings, new alignment, context, class logits [1, hyp, C]."""
        lm_state = self.tcn(inputs)[-1]
        att_state, att_weights = self.attn(att_state, lm_state, att_weights)
        context = torch.bmm(att_weights.t().unsqueeze(1), encoded.transpose(0, 1)).squeeze(1)
        logits = self._step_output(lm_state, context).unsqueeze(0)
        return logits, {'encoded': encoded, 'att_state': att_state, 'att_weights': att_weights}

    def _make_search(self, batch_size, device):
        plain = (batch_size, self.beam_size, device, self.num_classes, self.length_normalization)
        if not self.lm:
            return BeamSearch(*plain)
        fused = (self.lm, self.lm_weight, self.alphabet_mapping, self.min_attention_pos,
                 self.coverage_tau, self.coverage_weight) + plain
        if self.rescore:
            return RescoreSearchLM(self.rescore, *fused, keep_eos_score=self.keep_eos_score)
        if self.use_graph_search:
            return GraphSearch(self.hash_dec, self.graph_search_merge_threshold, *fused,
                               keep_eos_score=self.keep_eos_score)
        return BeamSearchLM(*fused, keep_eos_score=self.keep_eos_score)

    def _make_device_search(self, B, dev, lens, T):
        """The device search of this model for B utterances of at most T frames (`lens` on the
        device): DeviceBeamSearch, with an LM DeviceBeamSearchLM, with use_graph_search
        DeviceGraphSearch — or None, with `_native_gave_up` saying so, when the graph search
        refuses its node store (before anything is allocated)."""
        plain = (B, self.beam_size, dev, self.num_classes, self.length_normalization,
                 self.TRANSCRIPTION_LEN_GUARD)
        if not self.lm:
            return bs.DeviceBeamSearch(*plain)
        fused = (self.lm, self.lm_weight, self.alphabet_mapping, self.min_attention_pos,
                 self.coverage_tau, self.coverage_weight) + plain + (T, lens)
        if not self.use_graph_search:
            return bs.DeviceBeamSearchLM(*fused, keep_eos_score=self.keep_eos_score)
        try:
            return bs.DeviceGraphSearch(self.hash_dec, self.graph_search_merge_threshold,
                                        self._graph_span(), *fused,
                                        keep_eos_score=self.keep_eos_score)
        except bs.GraphStoreOverBudget as refused:
            self._native_gave_up = ('graph_store', refused.need, refused.budget)
            return None

    def _native_window_ok(self):
        """The device decode step takes no window, or a force_forward (lo, hi) of integers with
        lo < hi and hi >= 1 (asr_tcn_attention_step_win_f32; with hi < 1 the reference's
        `mask[right:]` takes a negative index, which stays with the torch path).
        ASR_TCN_FF_NATIVE=0, read per call, sends every windowed model to the torch path."""
        window = self.attn.force_forward
        if not window:
            return True
        if os.environ.get('ASR_TCN_FF_NATIVE', '1') == '0':
            return False
        try:
            lo, hi = window
        except (TypeError, ValueError):
            return False
        integral = all(isinstance(v, int) and not isinstance(v, bool) for v in (lo, hi))
        return integral and lo < hi and hi >= 1

    def _native_decode_ok(self, encoded):
        C, beam = self.num_classes, self.beam_size
        if os.environ.get('ASR_TCN_NATIVE', '1') == '0':     # A/B switch: torch ops + BeamSearch
            return False
        if self.lm and not self._native_lm_ok(encoded):
            return False
        return (encoded.is_cuda and not self.training
                and self._native_window_ok() and self.attn.kernel_size == 32
                and 1 <= encoded.size(0) <= _STEP_MAX_FRAMES and beam <= 32 and beam * (C - 1) <= 2048 and encoded.dtype == torch.float32)

    def _native_lm_ok(self, encoded):
        """The device LM-fused search (DeviceBeamSearchLM) takes a model with an LM when the LM's
        epsilon graph is acyclic, its labels fit the classes, neither rescore nor graph search is
        asked for, and a force_forward window is one the device step takes (_native_window_ok).
        ASR_LM_BEAM_NATIVE, read per call: 0 keeps the host
        BeamSearchLM (one utterance at a time), 1 takes the device search for every batch size;
        unset, batches go to the device and a single utterance stays with the host class, which is
        what it ran on before and against which the device search has not been timed yet.
        A model with use_graph_search takes the device path (DeviceGraphSearch) only with
        ASR_GRAPH_SEARCH_NATIVE=1, read per call, and then for every batch size, a single
        utterance included, unless ASR_LM_BEAM_NATIVE=0."""
        switch = os.environ.get('ASR_LM_BEAM_NATIVE', '')
        graph_native = bool(self.use_graph_search) and self._native_graph_ok(encoded)
        if switch == '0' or (switch != '1' and encoded.size(1) == 1 and not graph_native):
            return False
        if self.rescore or (self.use_graph_search and not graph_native) or not self._native_window_ok():
            return False
        if self.lm_weight == 0 and not self.coverage_weight > 0:
            return False
        return bool(encoded.is_cuda and self._lm_fits_device(encoded))

    def _lm_fits_device(self, encoded):
        """the LM's epsilon graph is acyclic, its labels fit the classes, its arrays the device"""
        lm = self.lm
        return not (lm.eps_rank() is None or not len(lm.ilabel)
                    or int(lm.ilabel.max()) >= self.num_classes
                    or lm.device_arrays(encoded.device) is None)

    def _graph_span(self):
        """the number of labels in GraphSearch's merge key (hash_dec)"""
        span = self.graph_search_history_len
        return self.tcn.eff_history if span < 0 else span

    def _native_graph_ok(self, encoded):
        """ASR_GRAPH_SEARCH_NATIVE=1 (read per call; off by default) and shapes the merge kernel takes."""
        if os.environ.get('ASR_GRAPH_SEARCH_NATIVE', '') != '1':
            return False
        from att_speech import _native
        return _native.graph_search_supported(self.beam_size, self._graph_span(), encoded.size(0))

    def _decode_native(self, encoded, encoded_lens, return_attention, poll_every=8):
        """The MI355X decode loop, for the plain beam search and, with an LM, the LM-fused one
        (DeviceBeamSearchLM: asr_lm_label_costs_f64, asr_beam_lm_step_f32, asr_lm_bag_advance_f64 in
        place of asr_beam_step_f32; with use_graph_search and ASR_GRAPH_SEARCH_NATIVE=1 the graph search,
        DeviceGraphSearch, which adds asr_graph_merge_f32; None when an LM bag outgrew the cap or the
        graph search's node store its budget, `_native_gave_up` says which): per label step the
        step body (_DeviceStepper.step) and ONE launch for the beam bookkeeping (asr_beam_step_f32)
        — no host read-back inside a step; the all-finished flag is polled every `poll_every`
        steps (steps behind the flag change nothing)."""
        from att_speech import _native
        T, B, E = encoded.shape
        beam, dev = self.beam_size, encoded.device
        lens = torch.as_tensor(encoded_lens).to(dev, torch.int32)
        self._native_gave_up = None
        search = self._make_device_search(B, dev, lens, T)
        if search is None:
            return None
        stepper = _DeviceStepper(self, encoded, lens)
        first = stepper.first
        att = first.t().repeat_interleave(beam, dim=0).contiguous()          # [hyp, T]
        history = stepper.empty_history(B * beam)
        parent = None
        trace_att = [first.repeat_interleave(beam, dim=1).detach()] if return_attention else None
        trace_logits = []
        for step in range(self.TRANSCRIPTION_LEN_GUARD):
            logits, att = stepper.step(history, att, parent, beam)
            chosen, parent = search.step(logits, att)
            if return_attention:
                trace_logits.append(logits.detach()[None])
                trace_att.append(att.t().detach())
            history = stepper.roll(history, parent, chosen)
            if (return_attention or step % poll_every == poll_every - 1) and search.poll_finished():
                break
        search.finalize()
        if getattr(search, 'overflow', 0):
            self._last_bag_overflow = search.overflow
            self._native_gave_up = ('lm_bag_overflow', search.overflow, _native.LM_BAG_CAP)
            return None                                  # an LM bag outgrew the device's cap
        return self._decode_result(search, return_attention, trace_att, trace_logits)

    @staticmethod
    def _decode_result(search, return_attention, trace_att, trace_logits):
        out = bs.best_result(search)
        if return_attention:
            out.update(attweights=trace_att, logits=trace_logits)
        out.update(coverage=search.coverage, graph=search.get_graph(), beam_search=search)
        return out

    def _warn_gave_up(self, prefix=''):
        """the device path returned None: say why (`_native_gave_up`), once per process and key"""
        from att_speech import _native
        why, asked, cap = self._native_gave_up
        if not _native._WARNED.get(prefix + why):
            _native._WARNED[prefix + why] = True
            warnings.warn(_GAVE_UP_WARNINGS[prefix + why] % (asked, cap))

    def _decode_host_each(self, encoded, encoded_lens, return_attention):
        """The host BeamSearchLM / GraphSearch takes one utterance per call: a batch whose device
        search gave up (an LM bag above the cap, a node store above the budget) is decoded utterance
        by utterance, each on its own frames, and the results are joined (lists over the utterances;
        `beam_search`, `coverage`, `attweights` and `logits` are lists of the per-utterance values,
        `graph` of the per-utterance graphs for a graph-search model, None otherwise)."""
        lens = [int(v) for v in torch.as_tensor(encoded_lens).tolist()]
        old = os.environ.get('ASR_LM_BEAM_NATIVE')
        os.environ['ASR_LM_BEAM_NATIVE'] = '0'
        try:
            parts = [self.decode(encoded[:lens[b], b:b + 1].contiguous(), torch.tensor([lens[b]]),
                                 return_attention=return_attention) for b in range(len(lens))]
        finally:
            if old is None:
                del os.environ['ASR_LM_BEAM_NATIVE']
            else:
                os.environ['ASR_LM_BEAM_NATIVE'] = old
        out = {'decoded': [p['decoded'][0] for p in parts],
               'decoded_scores': {k: [p['decoded_scores'][k][0] for p in parts]
                                  for k in parts[0]['decoded_scores']},
               'loss': torch.stack([p['loss'] for p in parts]).mean()}
        for k in ('attweights', 'logits', 'coverage', 'graph', 'beam_search'):
            if k in parts[0]:
                out[k] = [p[k] for p in parts]
        out['graph'] = [p['graph'][0] for p in parts] if self.use_graph_search else None
        return out

    def decode(self, encoded, encoded_lens, texts=None, text_lens=None,
               return_attention=False, print_debug=False, **kwargs):
        """Beam search over label steps (:476-585), at most TRANSCRIPTION_LEN_GUARD of them."""
        if self._native_decode_ok(encoded) and not print_debug:
            out = self._decode_native(encoded, encoded_lens, return_attention)
            if out is not None:
                return out
            self._warn_gave_up()
            if encoded.size(1) > 1:
                return self._decode_host_each(encoded, encoded_lens, return_attention)
        search = self._make_search(encoded.size(1), encoded.device)
        search.print_debug = print_debug
        state = self.enc_initial_state(encoded, encoded_lens, self.beam_size, encoded.size(1))
        trace_att = [state['att_weights'].detach()] if return_attention else None
        trace_logits = []
        for _ in range(self.TRANSCRIPTION_LEN_GUARD):
            history = state['inputs']
            logits, state = self.enc_step(**state)
            if return_attention:
                trace_logits.append(logits.detach())
                trace_att.append(state['att_weights'].detach())
            chosen, parent = search.step(logits, att_weights=state['att_weights'])
            # survivors inherit their parent's alignment and label history
            state['att_weights'] = state['att_weights'][:, parent]
            state['inputs'] = torch.cat((history[1:, parent], self.embedding(chosen)[None]))
            if search.has_finished():
                break
        return self._decode_result(search, return_attention, trace_att, trace_logits)

    # ---------------------------------------------------------------- forced scoring
    def _check_sentences(self, sentences, batch_size):
        if len(sentences) != batch_size:
            raise ValueError('score_sentences: %d sentence lists for %d utterances'
                             % (len(sentences), batch_size))
        for per_utt in sentences:
            for sent in per_utt:
                if len(sent) == 0:
                    raise ValueError('score_sentences: an empty sentence')
                for c in sent:
                    if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
                        raise ValueError('score_sentences: labels must be integers, got %r' % (c,))
                    if not 0 <= c < self.EOS:
                        raise ValueError('score_sentences: label %d outside [0, %d) (EOS is appended '
                                         'here)' % (c, self.EOS))

    def _native_forced_ok(self, encoded):
        """The device path of score_sentences (DeviceForcedScorer) takes what the decode step takes:
        a cuda fp32 encoder output of at most _STEP_MAX_FRAMES frames, 32 filter taps, no window or
        one the step accepts (_native_window_ok), and an LM, if any, whose epsilon graph is acyclic
        and whose labels fit the classes.  ASR_FORCED_NATIVE=0, read per call, keeps the host loop;
        the device path is the default at every size, a single sentence included (it measured
        1.6x the host loop there)."""
        if os.environ.get('ASR_FORCED_NATIVE', '1') == '0':
            return False
        if not (encoded.is_cuda and encoded.dtype == torch.float32 and self.attn.kernel_size == 32
                and 1 <= encoded.size(0) <= _STEP_MAX_FRAMES and 2 <= self.num_classes <= 2048
                and self._native_window_ok()):
            return False
        return self.lm is None or self._lm_fits_device(encoded)

    def _score_lm_host(self, sent):
        """score_lm of the scripts: the cost of the bag after the sentence and EOS"""
        bag = {self.lm.start(): 0}
        for c in list(sent) + [self.EOS]:
            bag = fst_utils.expand(self.lm, bag, self.alphabet_mapping[c], use_log_probs=True)
        return fst_utils.reduce_weights(bag.values(), True)

    def _score_sentences_host(self, encoded, lens, sentences):
        """The per-sentence loop of the scripts (score_acoustic / score_lm): every sentence on its
        own, batch 1, on the utterance's own frames; one read-back per sentence.
        -> per utterance (acoustic, covered frames, LM cost or None)."""
        out = []
        beam, self.beam_size = self.beam_size, 1        # enc_initial_state repeats lens by it
        try:
            for u, per_utt in enumerate(sentences):
                enc_u = encoded[:lens[u], u:u + 1].contiguous()
                acoustic, covered = np.zeros(len(per_utt)), np.zeros(len(per_utt), np.int64)
                lm = np.zeros(len(per_utt)) if self.lm is not None else None
                for j, sent in enumerate(per_utt):
                    state = self.enc_initial_state(enc_u, torch.tensor([lens[u]]), 1, 1)
                    cov = state['att_weights'].clone()
                    terms = []
                    for c in list(sent) + [self.EOS]:
                        history = state['inputs']
                        logits, state = self.enc_step(**state)
                        cov = cov + state['att_weights']
                        terms.append(F.log_softmax(logits[0, 0], dim=-1)[c])
                        new_input = torch.tensor([c], device=encoded.device)
                        state['inputs'] = torch.cat((history[1:], self.embedding(new_input)[None]))
                    k = (cov[:, 0] > self.coverage_tau).sum()
                    host = torch.cat((torch.stack(terms).double(), k.double()[None])).cpu().tolist()
                    acoustic[j] = sum(host[:-1])                  # fp64, in position order
                    covered[j] = int(host[-1])
                    if lm is not None:
                        lm[j] = self._score_lm_host(sent)
                out.append((acoustic, covered, lm))
        finally:
            self.beam_size = beam
        return out

    def _score_sentences_native(self, encoded, lens, sentences):
        """The device path: the sentences of every utterance as a prefix trie, one label step per
        trie LEVEL for all distinct prefixes of that length (_DeviceStepper.step, a level `width`
        rows per utterance, with the forced bookkeeping of DeviceForcedScorer behind it), nothing
        read back before the end.  None when an LM bag outgrew the device's cap."""
        from att_speech import _native
        T, B, E = encoded.shape
        dev = encoded.device
        tries = [bs.sentence_trie(per_utt, self.EOS) for per_utt in sentences]
        levels, offsets = bs.batch_trie_levels(tries)
        lens_dev = torch.as_tensor(lens).to(dev, torch.int32)
        scorer = bs.DeviceForcedScorer(levels, offsets[-1], B, dev, self.num_classes, T, lens_dev,
                                       self.coverage_tau, lm=self.lm,
                                       alphabet_mapping=self.alphabet_mapping)
        stepper = _DeviceStepper(self, encoded, lens_dev)
        att = att0 = stepper.first.t().contiguous()                            # [B, T]
        history = stepper.empty_history(B)
        for l, lv in enumerate(levels):
            if l:
                history = stepper.roll(history, scorer.index(l, 'parent', long=True),
                                       scorer.index(l, 'label', long=True))
            logits, att = stepper.step(history, att, scorer.index(l, 'parent'), lv['width'])
            scorer.step(logits, att, att_init=att0)
        acoustic, covered, lm, overflow = scorer.finish()
        if overflow:
            self._native_gave_up = ('lm_bag_overflow', overflow, _native.LM_BAG_CAP)
            return None
        out = []
        for u, t in enumerate(tries):
            pick = offsets[u] + t['inverse']
            out.append((acoustic[pick], covered[pick], lm[pick] if lm is not None else None))
        return out

    def score_sentences(self, encoded, encoded_lens, sentences, coverage='log_fraction'):
        """Teacher-forced scores of given sentences: `rescore2` of the reference's
        egs/wsj/local/lattice_search/rescore_lattices2.py (coverage='log_fraction') and
        score_groundtruth.py (coverage='count').  encoded [T', B, E]; `sentences` holds per utterance
        a list of label-id lists (no EOS, none empty, labels in [0, num_classes - 1)).  Every
        utterance is scored on its own encoded_lens[u] frames, as a batch-1 call would.  Returns per
        utterance a dict of fp64 arrays with one value per sentence, in the given order:
          acoustic  sum over the positions 0..n of log_softmax(logits_i)[y_i], y_n = EOS (fp32 terms,
                    summed in fp64 in position order);
          coverage  with k = the frames whose summed alignments (the initial one included) exceed
                    coverage_tau (returned as `covered`): coverage_weight * log(k / len), or
                    coverage_weight * k for 'count';
          lm        -lm_weight * cost of the LM bag after the sentence and EOS (0.0 without an LM);
          loss      (acoustic + coverage + lm) / n ** length_normalization.
        On the MI355X the sentences are scored through their prefix trie (_score_sentences_native);
        CPU models, ASR_FORCED_NATIVE=0 and the shapes the decode step refuses take the per-sentence
        host loop, as does a call in which an LM bag outgrows the device's cap (one warning)."""
        if coverage not in ('log_fraction', 'count'):
            raise ValueError("score_sentences: coverage must be 'log_fraction' or 'count'")
        if self.training:
            raise RuntimeError('score_sentences needs eval() mode')
        lens = [int(v) for v in torch.as_tensor(encoded_lens).tolist()]
        sentences = [[[c for c in sent] for sent in per_utt] for per_utt in sentences]
        self._check_sentences(sentences, encoded.size(1))
        total = sum(len(per_utt) for per_utt in sentences)
        with torch.no_grad():
            parts = None
            if total and self._native_forced_ok(encoded):
                parts = self._score_sentences_native(encoded, lens, sentences)
                if parts is None:
                    self._warn_gave_up('forced_')
            if parts is None:
                parts = self._score_sentences_host(encoded, lens, sentences)
        out = []
        for u, (acoustic, covered, lm_cost) in enumerate(parts):
            n = np.array([len(sent) for sent in sentences[u]], np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                if coverage == 'count':
                    cov = self.coverage_weight * covered.astype(np.float64)
                else:
                    cov = self.coverage_weight * np.log(covered / float(lens[u]))
                lm = -self.lm_weight * lm_cost if lm_cost is not None else np.zeros(len(n))
                loss = (acoustic + cov + lm) / n ** self.length_normalization
            out.append({'acoustic': acoustic, 'coverage': cov, 'lm': lm, 'loss': loss,
                        'covered': covered})
        return out
