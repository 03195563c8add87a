"""att_speech.modules.decoders.attention_decoder — the additive-attention + GRU label decoder
of the reference module of the same dotted name (att_speech/modules/decoders/
attention_decoder.py): `Attention` (:26-111) and `AttentionDecoderRNN` (:114-345).

Kept: constructor keywords, attribute names (they are checkpoint keys: `embedding`,
`attn.encoded_to_hidden`, `attn.rec_state_to_hidden`, `attn.hidden_to_score`, `rnn`,
`rnn_zero_state`, `output_to_logits`), the `forward` / `decode` signatures and returned dicts.

How it runs is this build's own.  On the MI355X the whole teacher-forced recurrence —
attention, context and GRU cell of every label position — is ONE autograd node
(`_AttentionGruScan`: asr_att_gru_scan_fwd_f32 / _bwd_f32, csrc/att_gru.hip) between two
batched products (the embedding half of the GRU's input projection in front, the output layer
behind), and the plain beam search decodes with one such launch (L = 1) and one
asr_beam_step_f32 launch per label step.  On CPU tensors, and wherever the kernels do not
apply (more GRU layers, `att_force_forward`, an LM), the per-position loop runs on torch ops.
"""
from __future__ import absolute_import, division, print_function

import os

import torch
import torch.nn.functional as F
from torch import nn

from att_speech.lm_fst import LmFst
from att_speech.modules.beam_search import BeamSearch, BeamSearchLM, GraphSearch, best_result
from att_speech.utils import get_mask

_MASKED = 1e5       # what a padding frame's score is lowered by


class Attention(nn.Module):
    """score_t = hidden_to_score(tanh(encoded_to_hidden(encoded_t) + rec_state_to_hidden(state)))
    over the frames of an utterance, softmax over time.  Alignments are `[T', B]`."""

    def __init__(self, encoded_size, rec_state_size, hidden_size, force_forward=None, **kwargs):
        super(Attention, self).__init__(**kwargs)
        self.encoded_to_hidden = nn.Linear(encoded_size, hidden_size)
        self.rec_state_to_hidden = nn.Linear(rec_state_size, hidden_size, bias=False)
        self.hidden_to_score = nn.Linear(hidden_size, 1)
        self.hidden_size = hidden_size
        with torch.no_grad():           # every frame weighs the same at the start of training
            self.hidden_to_score.weight.zero_()
        self.force_forward = force_forward

    def init_attention(self, encoded, encoded_lens):
        """encoded [T', B, E], lens [B] -> ((encoder term [T', B, A], padding scores [T', B]),
        initial alignment [T', B]: everything on frame 0)."""
        steps, batch = encoded.size(0), encoded.size(1)
        pad = (get_mask(encoded_lens, steps, batch_first=False) - 1.0) * _MASKED
        first = torch.zeros((steps, batch), device=encoded.device)
        first[0, :] = 1
        return (self.encoded_to_hidden(encoded), pad.to(encoded.device)), first

    def recompute_forward_mask(self, prev_att_weights, mask):
        """Padding scores plus the `force_forward` window: frames outside
        [peak + force_forward[0], peak + force_forward[1]) of the previous alignment are
        lowered by another 1e5, except for utterances whose previous peak is below 0.1."""
        steps = mask.size(0)
        peak_value, peak = torch.max(prev_att_weights, 0)
        left = peak + self.force_forward[0]
        right = peak + self.force_forward[1]
        # (a negative right edge counts from the end, as a slice bound does)
        right = torch.where(right < 0, (right + steps).clamp(min=0), right)
        t = torch.arange(steps, device=mask.device)[:, None]
        outside = ((t < left[None, :]) | (t >= right[None, :])) & (peak_value >= 0.1)[None, :]
        return mask - _MASKED * outside.to(mask.dtype)

    def forward(self, att_state, rnn_state, prev_att_weights):
        """rnn_state [B, H] (the first GRU layer's) -> (att_state, alignment [T', B])."""
        encoder_term, mask = att_state
        hidden = encoder_term + self.rec_state_to_hidden(rnn_state).unsqueeze(0)
        scores = self.hidden_to_score(torch.tanh(hidden)).squeeze(2)
        if self.force_forward:
            mask = self.recompute_forward_mask(prev_att_weights, mask)
        return att_state, F.softmax(scores + mask, 0)


class _AttentionGruScan(torch.autograd.Function):
    """All label positions of attention -> context -> GRU cell as one autograd node
    (asr_att_gru_scan_fwd_f32 / asr_att_gru_scan_bwd_f32).
    eproj [T', B, A], encoded [T', B, E], gx_emb [L, B, 3H] (embedding half of W_ih x + b_ih),
    w_ic [3H, E] (context half of W_ih), w_hh [3H, H], b_hh [3H], w_rec [A, H], w_score [A],
    b_score [1], h0 [B, H], lens [B] int32 -> alignments [L, B, T'], states [L, B, H].
    Saved: the alignments, states, contexts [L, B, E], one gate record (r, z, n, W_hn h + b_hn)
    per unit [L, B, 4H] and the state's attention term [L, B, A].  Every weight gradient is a
    plain reduction over (position, utterance) and is formed here, as one product each, from
    the per-position operands the backward kernel leaves."""

    @staticmethod
    def forward(ctx, eproj, encoded, gx_emb, w_ic, w_hh, b_hh, w_rec, w_score, b_score, h0, lens):
        from att_speech import _native
        eproj, encoded, gx_emb = eproj.contiguous(), encoded.contiguous(), gx_emb.contiguous()
        w_ic, w_hh, w_rec = w_ic.contiguous(), w_hh.contiguous(), w_rec.contiguous()
        w_score, h0 = w_score.contiguous(), h0.contiguous()
        att, states, ctxs, gates, rec = _native.att_gru_scan_fwd(
            eproj, encoded, lens, gx_emb, w_ic, w_hh, b_hh, w_rec, w_score, b_score, h0)
        ctx.save_for_backward(eproj, encoded, lens, w_ic, w_hh, w_rec, w_score, h0, att, states,
                              ctxs, gates, rec)
        ctx.set_materialize_grads(False)
        return att, states

    @staticmethod
    def backward(ctx, d_att, d_states):
        from att_speech import _native
        (eproj, encoded, lens, w_ic, w_hh, w_rec, w_score, h0, att, states, ctxs, gates,
         rec) = ctx.saved_tensors
        d_eproj, d_gates, d_ctx, d_rec, d_v, d_h0 = _native.att_gru_scan_bwd(
            eproj, encoded, lens, w_ic.t().contiguous(), w_hh.t().contiguous(),
            w_rec.t().contiguous(), w_score, h0, att, states, gates, rec, d_att, d_states)
        L, B, H = states.shape
        rows = L * B
        h_prev = torch.cat((h0[None], states[:-1])).view(rows, H)
        d_gi = d_gates[:, :, :3 * H]                                           # = d gx_emb
        d_gh = torch.cat((d_gates[:, :, :2 * H], d_gates[:, :, 3 * H:]), 2).view(rows, 3 * H)
        d_w_ic = d_gi.reshape(rows, 3 * H).t().mm(ctxs.view(rows, -1))
        d_w_hh = d_gh.t().mm(h_prev)
        d_b_hh = d_gh.sum(0)
        d_w_rec = d_rec.view(rows, -1).t().mm(h_prev)
        # d encoded[t, b] = sum_l a_l[b, t] d c_l[b]
        d_encoded = torch.bmm(att.permute(1, 2, 0), d_ctx.transpose(0, 1)).transpose(0, 1)
        # (the softmax is shift-invariant: the score bias gets no gradient)
        return (d_eproj, d_encoded, d_gi, d_w_ic, d_w_hh, d_b_hh, d_w_rec, d_v.sum(0),
                torch.zeros_like(w_score[:1]), d_h0, None)


class AttentionDecoderRNN(nn.Module):
    def __init__(self, sample_batch, num_classes, n_layers, hidden_size,
                 dropout_p, lm_file=None, lm_weight=1.0, min_attention_pos=0.3,
                 coverage_tau=0.1, coverage_weight=0.5, beam_size=1,
                 att_force_forward=None,
                 length_normalization=1.2, keep_eos_score=False,
                 use_graph_search=False, vocabulary=None, **kwargs):
        super(AttentionDecoderRNN, self).__init__(**kwargs)
        # sizes; the class inventory gets an end-of-sequence symbol behind the last class
        self.encoded_size = sample_batch["features"].size(2)
        self.n_layers, self.hidden_size = n_layers, hidden_size
        self.EOS, self.num_classes = num_classes, num_classes + 1
        # modules (attribute names are checkpoint keys)
        self.embedding = nn.Embedding(self.num_classes, hidden_size)
        self.dropout = nn.Dropout(dropout_p)             # (the reference never applies it)
        self.attn = Attention(self.encoded_size, hidden_size, hidden_size, att_force_forward)
        self.rnn = nn.GRU(hidden_size + self.encoded_size, hidden_size, n_layers,
                          dropout=dropout_p)
        self.rnn_zero_state = nn.Parameter(torch.zeros(n_layers, 1, hidden_size))
        self.output_to_logits = nn.Linear(hidden_size, self.num_classes)
        self.criterion = nn.NLLLoss(reduction='none')
        # search options
        self.beam_size = beam_size
        self.TRANSCRIPTION_LEN_GUARD = 400
        self.vocabulary = vocabulary
        self.lm = None
        if lm_file:
            assert vocabulary is not None
            self.lm = lm_file if isinstance(lm_file, LmFst) else LmFst.read(lm_file)
        self.alphabet_mapping = self.create_alphabet_mapping()
        self.lm_weight, self.min_attention_pos = lm_weight, min_attention_pos
        self.coverage_tau, self.coverage_weight = coverage_tau, coverage_weight
        self.length_normalization, self.keep_eos_score = length_normalization, keep_eos_score
        self.use_graph_search = use_graph_search

    def create_alphabet_mapping(self):
        """LM input label of every model class: by symbol name, the space as '<spc>'; classes
        the LM does not know — and EOS — also map to '<spc>'."""
        if self.lm is None:
            return None
        label_of = {sym: lab for lab, sym in self.lm.input_symbols()}
        names = ['<spc>' if s == ' ' else s for s in list(self.vocabulary) + ['<eos>']]
        return [label_of.get(name, label_of['<spc>']) for name in names]

    # ---------------------------------------------------------------- training
    def _native_train_ok(self, encoded):
        """The training recurrence through asr_att_gru_scan_*_f32 (read per call;
        ASR_ATT_RNN_NATIVE=0 keeps the per-position loop)."""
        if os.environ.get('ASR_ATT_RNN_NATIVE', '1') == '0':
            return False
        from att_speech import _native
        return (encoded.is_cuda and encoded.dtype == torch.float32 and self.n_layers == 1
                and not self.attn.force_forward
                and _native.att_gru_supported(encoded.size(0), self.attn.hidden_size,
                                              self.encoded_size, self.hidden_size))

    def _step(self, encoded, att_state, alignment, inputs, rnn_state):
        """One label position on torch ops -> (alignment, GRU output [1, B, H], new state)."""
        att_state, alignment = self.attn(att_state, rnn_state[0], alignment)
        context = (alignment.unsqueeze(2) * encoded).sum(0)
        output, rnn_state = self.rnn(torch.cat((inputs, context), 1).unsqueeze(0), rnn_state)
        return alignment, output, rnn_state

    def _forward_scan(self, encoded, encoded_lens, embedded, eproj):
        H = self.hidden_size
        rnn, attn = self.rnn, self.attn
        lens = torch.as_tensor(encoded_lens).to(encoded.device, torch.int32)
        previous = torch.cat((torch.zeros_like(embedded[:1]), embedded[:-1]))
        gx_emb = F.linear(previous, rnn.weight_ih_l0[:, :H], rnn.bias_ih_l0)     # [L, B, 3H]
        h0 = self.rnn_zero_state[0].repeat(encoded.size(1), 1)
        return _AttentionGruScan.apply(
            eproj, encoded, gx_emb, rnn.weight_ih_l0[:, H:], rnn.weight_hh_l0, rnn.bias_hh_l0,
            attn.rec_state_to_hidden.weight, attn.hidden_to_score.weight.reshape(-1),
            attn.hidden_to_score.bias, h0, lens)

    def forward(self, encoded, encoded_lens, texts, text_lens,
                return_att_weights=False, return_rnn_states=False, **kwargs):
        """Teacher-forced loss: encoded [T', B, E], texts [B, max_text_len]; every position's
        GRU input is the previous label's embedding (zeros first) and the attention context;
        cross-entropy over labels + EOS, padding (class 0) ignored."""
        dev = encoded.device
        B, L = texts.size(0), texts.size(1) + 1
        labels = torch.zeros(B, L, dtype=torch.long)
        labels[:, :L - 1] = texts.cpu().long()
        labels[torch.arange(B), torch.as_tensor(text_lens).long()] = self.EOS
        labels = labels.to(dev)
        embedded = self.embedding(labels.t())                                   # [L, B, H]
        att_state, alignment = self.attn.init_attention(encoded, encoded_lens)
        if self._native_train_ok(encoded):
            att, states = self._forward_scan(encoded, encoded_lens, embedded, att_state[0])
            outputs = states
            alignments = [a.t() for a in att.unbind(0)] if return_att_weights else None
            rnn_states = [s.detach()[None] for s in states.unbind(0)] if return_rnn_states else None
        else:
            rnn_state = self.rnn_zero_state.repeat(1, B, 1)
            inputs = embedded.new_zeros(B, self.hidden_size)
            outputs, alignments, rnn_states = [], [], []
            for targets in embedded:
                alignment, output, rnn_state = self._step(encoded, att_state, alignment, inputs,
                                                          rnn_state)
                alignments.append(alignment)
                outputs.append(output)
                rnn_states.append(rnn_state.detach())
                inputs = targets
            outputs = torch.cat(outputs)
        logits = self.output_to_logits(outputs).permute(1, 0, 2).contiguous()   # [B, L, C]
        loss = F.cross_entropy(logits.view(B * L, -1), labels.view(B * L), ignore_index=0)
        ret = {'loss': loss}
        if return_att_weights:
            ret['attweights'] = alignments
        if return_rnn_states:
            ret['rnnstates'] = rnn_states
        return ret

    # ---------------------------------------------------------------- decoding
    def _make_search(self, batch_size, device):
        plain = (batch_size, self.beam_size, device, self.num_classes, self.length_normalization)
        if not self.lm:
            return BeamSearch(*plain)
        fused = (self.lm, self.lm_weight, self.alphabet_mapping, self.min_attention_pos,
                 self.coverage_tau, self.coverage_weight) + plain
        if self.use_graph_search:
            # the reference hands `self.hash_dec` to GraphSearch and this class has none
            return GraphSearch(self.hash_dec, *fused, keep_eos_score=self.keep_eos_score)
        return BeamSearchLM(*fused, keep_eos_score=self.keep_eos_score)

    def _native_decode_ok(self, encoded):
        C, beam = self.num_classes, self.beam_size
        if os.environ.get('ASR_ATT_RNN_NATIVE', '1') == '0':   # A/B switch: torch ops + BeamSearch
            return False
        from att_speech import _native
        return (encoded.is_cuda and encoded.dtype == torch.float32 and not self.lm
                and not self.training and not self.attn.force_forward and self.n_layers == 1
                and beam <= 32 and beam * (C - 1) <= 2048
                and _native.att_gru_supported(encoded.size(0), self.attn.hidden_size,
                                              self.encoded_size, self.hidden_size))

    def _decode_native(self, encoded, encoded_lens, poll_every=8):
        """The MI355X decode loop of the plain beam search: per label step ONE launch for
        attention + context + GRU cell of every hypothesis (asr_att_gru_scan_fwd_f32 with
        L = 1; hypothesis i reads the encoder operands of utterance i // beam, nothing is
        repeated per hypothesis), the output layer, ONE launch for the beam bookkeeping
        (asr_beam_step_f32), two gathers for the survivors' states and next inputs — no host
        read-back inside a step; the all-finished flag is polled every `poll_every` steps
        (steps behind the flag change nothing).  The previous alignment is not carried: only
        `att_force_forward` reads it, and that stays on the torch path."""
        from att_speech import _native
        from att_speech.modules.beam_search import DeviceBeamSearch
        H, beam, dev = self.hidden_size, self.beam_size, encoded.device
        B = encoded.size(1)
        rnn, attn = self.rnn, self.attn
        lens = torch.as_tensor(encoded_lens).to(dev, torch.int32)
        search = DeviceBeamSearch(B, beam, dev, self.num_classes, self.length_normalization,
                                  self.TRANSCRIPTION_LEN_GUARD)
        with torch.no_grad():
            enc = encoded.contiguous()
            eproj = attn.encoded_to_hidden(enc).contiguous()
            w_ih = rnn.weight_ih_l0
            # embedding half of the input projection of every class, once per decode
            table = F.linear(self.embedding.weight, w_ih[:, :H], rnn.bias_ih_l0)     # [C, 3H]
            w_ic = w_ih[:, H:].contiguous()
            w_score = attn.hidden_to_score.weight.reshape(-1).contiguous()
            h = self.rnn_zero_state[0].repeat(B * beam, 1)
            gx = rnn.bias_ih_l0.repeat(B * beam, 1)               # the first input is zero
            for step in range(self.TRANSCRIPTION_LEN_GUARD):
                _, states, _, _, _ = _native.att_gru_scan_fwd(
                    eproj, enc, lens, gx[None], w_ic, rnn.weight_hh_l0, rnn.bias_hh_l0,
                    attn.rec_state_to_hidden.weight, w_score, attn.hidden_to_score.bias, h,
                    beam=beam, save=False)
                chosen, parent = search.step(self.output_to_logits(states[0]))
                h = states[0].index_select(0, parent.long())
                gx = table.index_select(0, chosen.long())
                if step % poll_every == poll_every - 1 and search.poll_finished():
                    break
        search.finalize()
        return best_result(search)

    def decode(self, encoded, encoded_lens, texts=None, text_lens=None, print_debug=False,
               **kwargs):
        """Beam search over label steps, at most TRANSCRIPTION_LEN_GUARD of them; the
        hypotheses of an utterance are adjacent."""
        if self._native_decode_ok(encoded) and not print_debug:
            return self._decode_native(encoded, encoded_lens)
        B, beam = encoded.size(1), self.beam_size
        search = self._make_search(B, encoded.device)
        search.print_debug = print_debug
        per_hyp = encoded.repeat_interleave(beam, dim=1)
        lens = torch.as_tensor(encoded_lens).repeat_interleave(beam)
        att_state, alignment = self.attn.init_attention(per_hyp, lens)
        rnn_state = self.rnn_zero_state.repeat(1, B, 1).repeat_interleave(beam, dim=1)
        inputs = encoded.new_zeros(B * beam, self.hidden_size)
        for _ in range(self.TRANSCRIPTION_LEN_GUARD):
            alignment, output, rnn_state = self._step(per_hyp, att_state, alignment, inputs,
                                                      rnn_state)
            chosen, parent = search.step(self.output_to_logits(output), att_weights=alignment)
            inputs = self.embedding(chosen)
            rnn_state = rnn_state[:, parent]
            alignment = alignment[:, parent]
            if search.has_finished():
                break
        return best_result(search)

    def single_step(self, word_input, last_hidden, encoder_outputs, encoded_lens,
                    precomputed_V_enc_out):
        pass
