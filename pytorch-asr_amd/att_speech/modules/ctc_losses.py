"""att_speech.modules.ctc_losses — loss front-ends of the reference
(att_speech/modules/ctc_losses.py) on the MI355X kernels.

Kept: get_normalized_acts (:29-43), ctc_loss (:46-64, evaluated with the
lattice kernel instead of F.ctc_loss, same 'mean' reduction), ctc_fst_loss
(:617-657), and ctc_raw_loss / ctc_raw_loss_batch (:521-609) as front-ends of the
same sparse lattice kernel: the reference evaluates those two with dense
[N, N] transition matrices (RawGenericCTC*, :268-390, O(T N^2)); the value is the
same sum over alignments, so no dense path is built here — the dense
arithmetic lives in the golden fixtures as an independent oracle.

Alignment (:67-265, :412-518): the dense builders get_CTC_matrices_* /
get_CTC_decoding_matrices_*, raw_generic_viterbi and the mono / bi align and decode
functions are restated on the host (numpy, fp64 accumulator, first-index ties);
ctc_viterbi_align_batch aligns a whole batch, on a device tensor with one launch of
asr_ctc_align_f64 (csrc/ctc_align.hip, bit-identical to the host path)."""
from __future__ import absolute_import, division, print_function

import collections
import os

import numpy as np
import torch

from att_speech import _native
from att_speech.fst_utils import CTCGraphGen, path_reduction, path_logsumexp  # noqa: F401


class _GroupLogSoftmax(torch.autograd.Function):
    """log_softmax over contiguous groups of `group` classes (HIP fwd + bwd)."""

    @staticmethod
    def forward(ctx, acts, group):
        y = _native.log_softmax_fwd(acts.contiguous(), group)
        ctx.save_for_backward(y)
        ctx.group = group
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _native.log_softmax_bwd(y, dy.contiguous(), ctx.group), None


def get_normalized_acts(acts, acts_lens, num_symbols, context_order,
                        normalize_by_dim, normalize_logits=True):
    """reference ctc_losses.py:29-43.  normalize_by_dim > 0 normalises over
    axis normalize_by_dim + 2 of the [T,B,S,...,S] view.  The last axis (contiguous
    groups of S: what the shipped configs use) goes straight to the group kernel; any
    other axis (context_order >= 3) is moved to the end, normalised there and moved back."""
    assert context_order == 1 or num_symbols
    del acts_lens  # unused
    if normalize_by_dim:
        assert acts.size(-1) == num_symbols ** context_order
        if not 0 < normalize_by_dim < context_order:
            raise IndexError("normalize_by_dim=%d: the [T,B,S,...] view of context_order %d has "
                             "no axis %d" % (normalize_by_dim, context_order, normalize_by_dim + 2))
        if normalize_by_dim == context_order - 1:
            return _GroupLogSoftmax.apply(acts, num_symbols)
        size = acts.size()
        v = acts.view(*(tuple(size[:2]) + (num_symbols,) * context_order))
        v = v.movedim(normalize_by_dim + 2, -1).contiguous()
        y = _GroupLogSoftmax.apply(v.view(size[0], size[1], -1), num_symbols)
        return y.view(v.shape).movedim(-1, normalize_by_dim + 2).contiguous().view(size)
    elif normalize_logits:
        return _GroupLogSoftmax.apply(acts, acts.size(-1))
    return acts


def _labels_to_batch(labels, label_lens):
    """flat concatenated labels -> padded [B, Lmax] (reference :646-652)."""
    label_lens = torch.as_tensor(label_lens)
    lab = torch.zeros((label_lens.numel(), int(label_lens.max()) if label_lens.numel() else 0),
                      dtype=torch.int64)
    ls = 0
    for b in range(label_lens.numel()):
        le = ls + int(label_lens[b])
        lab[b, :le - ls] = torch.as_tensor(labels[ls:le]).long()
        ls = le
    return lab


_graph_gens = {}


def _graph_gen(num_symbols, context_order, **graph_build_args):
    key = (num_symbols, context_order, tuple(sorted(graph_build_args.items())))
    if key not in _graph_gens:
        _graph_gens[key] = CTCGraphGen(
            context_order=context_order, num_symbols=num_symbols,
            for_forward_only=False, graph_build_args=graph_build_args)
    return _graph_gens[key]


def ctc_fst_loss(acts, labels, act_lens, label_lens,
                 num_symbols=0, context_order=1, normalize_by_dim=None,
                 allow_nonblank_selfloops=True,
                 loop_using_symbol_repetitions=False,
                 other_data_in_batch=None,
                 eval_repeats_in_context=False,
                 neg_inf=-1e20):
    """reference ctc_losses.py:617-657: per-utterance -log p(labels | acts)."""
    log_probs = get_normalized_acts(acts, act_lens, num_symbols,
                                    context_order, normalize_by_dim,
                                    normalize_logits=True)
    assert not (eval_repeats_in_context and loop_using_symbol_repetitions)
    S = log_probs.size(2)
    if other_data_in_batch and 'graph_matrices' in other_data_in_batch:
        graph_matrices = other_data_in_batch['graph_matrices']
    else:
        gg_kwargs = {}
        if context_order == 2:
            S = int(round(np.sqrt(S)))
            gg_kwargs = dict(
                allow_nonblank_selfloops=allow_nonblank_selfloops,
                loop_using_symbol_repetitions=loop_using_symbol_repetitions,
                eval_repeats_in_context=eval_repeats_in_context)
        graph_gen = _graph_gen(S, context_order, **gg_kwargs)
        labels_b = _labels_to_batch(labels, label_lens)
        graph_matrices = graph_gen.get_training_matrices_batch(labels_b, label_lens)
    return path_reduction(log_probs, act_lens, graph_matrices, neg_inf=neg_inf, negate=True)


def ctc_loss(acts, labels, act_lens, label_lens,
             num_symbols=None, context_order=1, normalize_by_dim=None,
             allow_nonblank_selfloops=True,
             loop_using_symbol_repetitions=False,
             eval_repeats_in_context=False,
             other_data_in_batch=None):
    """reference ctc_losses.py:46-64 — F.ctc_loss(log_softmax(acts), ...,
    reduction='mean'): per-utterance losses divided by the target lengths,
    then averaged.  Evaluated with the mono CTC lattice (identical value,
    SURVEY.md §4) instead of the vendor CTC."""
    for condition in [context_order == 1,
                      normalize_by_dim is None,
                      not eval_repeats_in_context,
                      allow_nonblank_selfloops,
                      not loop_using_symbol_repetitions,
                      not other_data_in_batch]:
        assert condition, "Option not supported in this loss"
    assert acts.size(0) == act_lens[0]
    assert int(torch.as_tensor(labels).max()) < acts.size(2)
    losses = ctc_fst_loss(acts, labels, act_lens, label_lens,
                          num_symbols=acts.size(2), context_order=1,
                          normalize_by_dim=None)
    # an utterance with no feasible alignment: the lattice returns -neg_inf-sized values,
    # F.ctc_loss(zero_infinity=False) returns inf (and the mean with it)
    losses = torch.where(losses >= 5e19, torch.full_like(losses, float('inf')), losses)
    tl = torch.as_tensor(label_lens).to(losses.device, losses.dtype).clamp(min=1)
    return (losses / tl).mean()


def ctc_raw_loss_batch(acts, labels, act_lens, label_lens,
                       num_symbols=0, context_order=1, normalize_by_dim=None,
                       allow_nonblank_selfloops=True,
                       loop_using_symbol_repetitions=False,
                       eval_repeats_in_context=False,
                       other_data_in_batch=None,
                       **kwargs):
    """reference ctc_losses.py:563-609 — per-utterance CTC losses over the dense
    mono / bicontext transition matrices (get_CTC_matrices_mono :67-94,
    get_CTC_matrices_bicontext :111-166).  Same alignments as the sparse training
    lattice of CTCGraphGen, so it is evaluated with the lattice kernel.  The bicontext
    matrices with eval_repeats_in_context=False treat a repeated symbol differently
    from the FST lattice; that combination is refused for label
    sequences that contain a repeat instead of returning a different number."""
    assert not other_data_in_batch
    assert not (eval_repeats_in_context and loop_using_symbol_repetitions)
    if kwargs:
        raise NotImplementedError("ctc_raw_loss: unsupported options %s" % sorted(kwargs))
    if context_order == 1:
        assert not loop_using_symbol_repetitions
        return ctc_fst_loss(acts, labels, act_lens, label_lens, num_symbols=num_symbols,
                            context_order=1, normalize_by_dim=normalize_by_dim)
    assert context_order == 2 and normalize_by_dim == 1 and num_symbols > 0
    if loop_using_symbol_repetitions:
        raise NotImplementedError("loop_using_symbol_repetitions lattices are not built")
    if not eval_repeats_in_context:
        flat = torch.as_tensor(labels).long().cpu() % num_symbols
        ends = torch.as_tensor(label_lens).long().cpu().cumsum(0).tolist()
        start = 0
        for end in ends:
            seq = flat[start:end]
            if seq.numel() > 1 and bool((seq[1:] == seq[:-1]).any()):
                raise NotImplementedError(
                    "dense bicontext CTC with eval_repeats_in_context=False on a label "
                    "sequence with a repeated symbol differs from the FST lattice")
            start = end
    # the bicontext matrices emit a CONTEXT-SPECIFIC blank before each symbol
    # (get_CTC_matrices_bicontext, :123-166): the training lattice with contextual blanks
    log_probs = get_normalized_acts(acts, act_lens, num_symbols, 2, normalize_by_dim,
                                    normalize_logits=True)
    graph_gen = _graph_gen(num_symbols, 2, allow_nonblank_selfloops=allow_nonblank_selfloops,
                           use_contextual_blanks=True)
    graph_matrices = graph_gen.get_training_matrices_batch(
        _labels_to_batch(labels, label_lens), label_lens)
    return path_reduction(log_probs, act_lens, graph_matrices, negate=True)


# the reference's per-utterance Python loop (:521-560) computes the same values
ctc_raw_loss = ctc_raw_loss_batch


# ----------------------------------------------------------------------------
# Forced alignment and frame-level Viterbi decoding (reference :67-265, :412-518)
# ----------------------------------------------------------------------------
def _label_list(L, S=None):
    seq = [int(v) for v in torch.as_tensor(L).reshape(-1).tolist()]
    return seq if S is None else [v % S for v in seq]


def get_CTC_matrices_mono(L, S):
    """reference :67-94 — (A [N,N], B [S,N]) of the mono CTC lattice of the labels L:
    N = 2 len(L) + 1, even states emit the blank (class 0), state 2i+1 emits L[i]; every
    state loops, each state enters the next, and label i enters label i+1 directly when
    the two differ."""
    seq = _label_list(L)
    N = 2 * len(seq) + 1
    A, B = torch.zeros(N, N), torch.zeros(S, N)
    idx = torch.arange(N)
    A[idx, idx] = 1.0
    A[idx[:-1], idx[1:]] = 1.0
    B[0, 0::2] = 1.0
    for i, l in enumerate(seq):
        B[l, 2 * i + 1] = 1.0
        if i + 1 < len(seq) and seq[i + 1] != l:
            A[2 * i + 1, 2 * i + 3] = 1.0
    return A, B


def get_CTC_decoding_matrices_mono(S):
    """reference :97-108 — any class follows any class, class s emits s."""
    return torch.ones(S, S), torch.eye(S, S)


def get_CTC_matrices_bicontext_looprepeats(L, S):
    """reference :169-226 — three states per label (entry in the old context, a looping copy
    in its own context, its contextual blank): N = 3 len(L) + 1."""
    seq = _label_list(L, S)
    N = 3 * len(seq) + 1
    A, B = torch.zeros(N, N), torch.zeros(S ** 2, N)
    B[0, 0] = 1.0
    A[0, 0] = A[0, 1] = 1.0
    ctx = 0
    for i, l in enumerate(seq):
        entry, loop, blank, nxt = 3 * i + 1, 3 * i + 2, 3 * i + 3, 3 * i + 4
        B[ctx * S + l, entry] = 1.0
        ctx = l
        B[ctx * S + l, loop] = 1.0
        B[ctx * S, blank] = 1.0
        to_next = i + 1 < len(seq) and l != seq[i + 1]
        for src in (entry, loop):
            A[src, loop] = A[src, blank] = 1.0
            if to_next:
                A[src, nxt] = 1.0
        A[blank, blank] = 1.0
        if i + 1 < len(seq):
            A[blank, nxt] = 1.0
    return A, B


def get_CTC_matrices_bicontext(L, S, eval_repeats_in_context=False,
                               allow_nonblank_selfloops=True,
                               loop_using_symbol_repetitions=False):
    """reference :111-166 — the bicontext lattice (labels reduced modulo S): the blank before
    label i emits class ctx_i * S and the label ctx_i * S + L[i], with ctx_0 = 0 and
    ctx_{i+1} = L[i]; the last blank emits L[-1] * S.  Labels loop only with
    allow_nonblank_selfloops; label i enters label i+1 directly unless the repeat test fires
    (L[i] == L[i+1], or with eval_repeats_in_context the two emitted classes being equal)."""
    if loop_using_symbol_repetitions:
        assert not eval_repeats_in_context
        return get_CTC_matrices_bicontext_looprepeats(L, S)
    seq = _label_list(L, S)
    N = 2 * len(seq) + 1
    A, B = torch.zeros(N, N), torch.zeros(S ** 2, N)
    ctx = 0
    for i, l in enumerate(seq):
        blank, tok = 2 * i, 2 * i + 1
        B[ctx * S, blank] = 1.0
        B[ctx * S + l, tok] = 1.0
        A[blank, blank] = A[blank, tok] = A[tok, tok + 1] = 1.0
        if allow_nonblank_selfloops:
            A[tok, tok] = 1.0
        if i + 1 < len(seq):
            if eval_repeats_in_context:
                repeat = ctx * S + l == l * S + seq[i + 1]
            else:
                repeat = l == seq[i + 1]
            if not repeat:
                A[tok, tok + 2] = 1.0
        ctx = l
    B[ctx * S, N - 1] = 1.0
    A[N - 1, N - 1] = 1.0
    return A, B


def get_CTC_decoding_matrices_bicontext(S, eval_repeats_in_context=False,
                                        allow_nonblank_selfloops=True):
    """reference :229-265 — allowed class-to-class moves of the bicontext decoder, indexed
    (context, symbol) -> (context, symbol): a blank keeps its context, a symbol becomes the
    context of what follows, a symbol may repeat in place, and without
    eval_repeats_in_context a symbol never moves to itself under another context."""
    assert allow_nonblank_selfloops, "Case for False not implemented"
    A = torch.zeros(S, S, S, S)
    for c in range(S):
        A[c, 0, c, :] = 1.0
    for sym in range(1, S):
        A[:, sym, sym, :] = 1.0
        if not eval_repeats_in_context:
            A[:, sym, :, sym] = 0.0
        for c in range(S):
            A[c, sym, c, sym] = 1.0
    return A.view(S ** 2, S ** 2), torch.eye(S ** 2, S ** 2)


def _dense_viterbi_states(log_probs, A, B, start_states, terminal_states):
    """(cost, state path [T]) of the best path: float64 alphas, one addition of a float32
    log-prob per frame, np.argmax's first maximum over the source states."""
    T, S = log_probs.shape
    N = A.shape[0]
    assert A.shape == (N, N) and B.shape == (S, N)
    assert np.all(np.asarray(B.sum(0)) == 1)
    with np.errstate(divide='ignore'):
        lA = np.log(A)
    emit = log_probs.dot(B)                     # float32; exact, B is one-hot per state
    alpha = np.full((T, N), -np.inf)            # float64
    alpha[0] = emit[0]
    if start_states is not None:
        gate = np.full(N, -np.inf)
        gate[list(start_states)] = 0
        alpha[0] += gate
    back = np.zeros((T, N), np.int64)
    cols = np.arange(N)
    for t in range(1, T):
        cand = alpha[t - 1][:, None] + lA
        back[t] = cand.argmax(0)
        alpha[t] = cand[back[t], cols] + emit[t]
    if terminal_states is not None:
        gate = np.full(N, -np.inf)
        gate[list(terminal_states)] = 0
        alpha[-1] += gate
    path = np.empty(T, np.int64)
    path[-1] = alpha[-1].argmax()
    cost = -alpha[-1][path[-1]]
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t][path[t]]
    return cost, path


def raw_generic_viterbi(log_probs, A, B, start_states=None, terminal_states=None):
    """reference :412-457 — (cost, sol): minus the log-probability of the best state path
    through (A, B) and the class emitted at each frame (IntTensor [T]).  The log-probs must be
    finite: the emission product turns a -inf into NaN, in the reference as here."""
    lp = torch.as_tensor(log_probs).detach().cpu().numpy()
    Bn = torch.as_tensor(B).detach().cpu().numpy()
    cost, path = _dense_viterbi_states(lp, torch.as_tensor(A).detach().cpu().numpy(), Bn,
                                       start_states, terminal_states)
    return cost, torch.from_numpy(Bn.argmax(0)[path].astype(np.int32))


def _route_single(log_probs, labels, context_order, num_symbols, **flags):
    """(cost, sol) of one device utterance through the batch entry"""
    res = ctc_viterbi_align_batch(log_probs.unsqueeze(1), torch.as_tensor(labels).reshape(-1),
                                  [log_probs.size(0)], [torch.as_tensor(labels).numel()],
                                  num_symbols=num_symbols, context_order=context_order, **flags)
    cost = np.float64(res.cost[0].item())
    if res.feasible[0]:
        return cost, res.frames[0].cpu()
    # no alignment exists: the reference walks back-pointers of unreachable states here
    return cost, torch.zeros(log_probs.size(0), dtype=torch.int32)


def mono_CTC_viterbi_align(log_probs, labels):
    """reference :475-481 — align log_probs [T, S] to labels; a device tensor goes through
    ctc_viterbi_align_batch with one utterance."""
    if log_probs.is_cuda:
        return _route_single(log_probs, labels, 1, log_probs.size(1))
    A, B = get_CTC_matrices_mono(labels, log_probs.size(1))
    N = A.size(0)
    return raw_generic_viterbi(log_probs, A, B, start_states=[0, 1], terminal_states=[N - 2, N - 1])


def mono_CTC_viterbi_decode(log_probs):
    """reference :484-489 — frame-level best classes (no blank or repeat removal)."""
    A, B = get_CTC_decoding_matrices_mono(log_probs.size(1))
    return raw_generic_viterbi(log_probs, A, B, start_states=None, terminal_states=None)


def bi_CTC_viterbi_align(log_probs, labels, **kwargs):
    """reference :505-511 — align log_probs [T, S*S] to labels over the bicontext lattice."""
    S = int(np.sqrt(log_probs.size(1)))
    if log_probs.is_cuda and not kwargs.get('loop_using_symbol_repetitions'):
        return _route_single(log_probs, labels, 2, S, **kwargs)
    A, B = get_CTC_matrices_bicontext(labels, S, **kwargs)
    N = A.size(0)
    return raw_generic_viterbi(log_probs, A, B, start_states=[0, 1], terminal_states=[N - 2, N - 1])


def bi_CTC_viterbi_decode(log_probs, **kwargs):
    """reference :514-518 — frame-level best classes that respect the contexts."""
    S = int(np.sqrt(log_probs.size(1)))
    A, B = get_CTC_decoding_matrices_bicontext(S, **kwargs)
    return raw_generic_viterbi(log_probs, A, B, start_states=range(S), terminal_states=None)


CTCAlignment = collections.namedtuple('CTCAlignment', 'cost frames states segments feasible')


def _band_topology(seq, S, context_order, allow_nonblank_selfloops, eval_repeats_in_context):
    """class, self-loop flag and skip flag (entered from n - 2) of the 2 L + 1 states"""
    L = len(seq)
    N = 2 * L + 1
    cls, loop, skip = np.zeros(N, np.int64), np.ones(N, bool), np.zeros(N, bool)
    if context_order == 1:
        lab = np.asarray(seq, np.int64)
        cls[1::2] = lab
        skip[3::2] = lab[1:] != lab[:-1]
        return cls, loop, skip
    lab = np.asarray(seq, np.int64) % S
    ctx = np.concatenate([[0], lab])                # ctx[i]: context of label i; ctx[L]: of the last blank
    cls[0::2] = ctx * S
    cls[1::2] = ctx[:-1] * S + lab
    loop[1::2] = bool(allow_nonblank_selfloops)
    if eval_repeats_in_context:
        repeat = ctx[:-2] * S + lab[:-1] == lab[:-1] * S + lab[1:]
    else:
        repeat = lab[:-1] == lab[1:]
    skip[3::2] = ~repeat
    return cls, loop, skip


def _band_viterbi(lp, seq, S, context_order, allow_nonblank_selfloops, eval_repeats_in_context):
    """One utterance on the host over the three-predecessor band: the additions and the
    first-maximum rule of _dense_viterbi_states without the [N, N] matrix.  lp [T, C] float32.
    Returns (cost, states [T]) or (inf, None)."""
    T = lp.shape[0]
    if T == 0 or len(seq) == 0:
        return np.inf, None
    cls, loop, skip = _band_topology(seq, S, context_order, allow_nonblank_selfloops,
                                     eval_repeats_in_context)
    N = cls.size
    emit = lp[:, cls]                               # float32 [T, N]
    alpha = np.full(N, -np.inf)
    alpha[:2] = emit[0, :2]
    back = np.zeros((T, N), np.int8)
    cand = np.empty((3, N))
    ninf = -np.inf
    for t in range(1, T):
        cand[0, :2] = ninf
        cand[0, 2:] = np.where(skip[2:], alpha[:-2], ninf)
        cand[1, 0] = ninf
        cand[1, 1:] = alpha[:-1]
        cand[2] = np.where(loop, alpha, ninf)
        k = cand.argmax(0)                          # ascending source order, first maximum
        back[t] = 2 - k
        alpha = cand[k, np.arange(N)] + emit[t]
    st = N - 1 if alpha[N - 1] > alpha[N - 2] else N - 2
    if not alpha[st] > -np.inf:
        return np.inf, None
    states = np.empty(T, np.int32)
    for t in range(T - 1, -1, -1):
        states[t] = st
        st -= int(back[t][st])
    return -alpha[states[-1]], states


def _align_native_enabled():
    return os.environ.get('ASR_ALIGN_NATIVE', '1') != '0'


def ctc_viterbi_align_batch(log_probs, labels, act_lens, label_lens,
                            num_symbols=0, context_order=1,
                            allow_nonblank_selfloops=True,
                            eval_repeats_in_context=False):
    """Forced alignment of a batch: the best path of every utterance through its mono
    (context_order 1) or bicontext (2) CTC lattice, i.e. mono_CTC_viterbi_align /
    bi_CTC_viterbi_align on log_probs[:act_lens[b], b] and the b-th transcript.

    log_probs [T, B, C] float32, finite (see raw_generic_viterbi); labels: the transcripts
    concatenated, as the loss functions take them; act_lens (any order) and label_lens [B].
    Returns CTCAlignment(cost [B] f64, frames [B, T] i32 = class per frame, states [B, T] i32
    = lattice state per frame, segments [B, Lmax, 2] i32 = (first frame, one past the last)
    of every label, feasible [B] bool), on the device of log_probs.  Padding is -1; an
    utterance with no alignment (too few frames, no frames, no labels) has cost inf,
    feasible False and -1 everywhere.

    A device tensor takes one launch of asr_ctc_align_f64 for the whole batch; CPU tensors,
    transcripts longer than the kernel is built for (511) and ASR_ALIGN_NATIVE=0 (read per
    call) take the host path.  Both give the same bits."""
    assert context_order in (1, 2)
    assert log_probs.dim() == 3 and log_probs.dtype == torch.float32
    T, B, C = log_probs.shape
    S = int(num_symbols) if num_symbols else (C if context_order == 1 else int(round(np.sqrt(C))))
    assert context_order == 1 or S * S <= C
    act = [int(v) for v in torch.as_tensor(act_lens).reshape(-1).tolist()]
    lls = [int(v) for v in torch.as_tensor(label_lens).reshape(-1).tolist()]
    assert len(act) == B and len(lls) == B
    assert all(0 <= v <= T for v in act) and all(v >= 0 for v in lls)
    flat = torch.as_tensor(labels).reshape(-1).cpu().long()
    assert flat.numel() >= sum(lls)
    if flat.numel():
        assert int(flat.min()) >= 0 and (context_order == 2 or int(flat.max()) < C)
    padded = _labels_to_batch(flat, lls)
    Lmax = padded.size(1)
    dev = log_probs.device
    if (log_probs.is_cuda and _align_native_enabled() and B > 0
            and _native.ctc_align_supported(T, Lmax, C)):
        cost, frames, states, segments = _native.ctc_align(
            log_probs.detach(), torch.tensor(act, dtype=torch.int32, device=dev),
            padded.to(device=dev, dtype=torch.int32), torch.tensor(lls, dtype=torch.int32, device=dev),
            S, context_order, allow_nonblank_selfloops, eval_repeats_in_context)
        return CTCAlignment(cost, frames, states, segments, torch.isfinite(cost))
    lp = log_probs.detach().cpu().numpy()
    cost = np.full(B, np.inf)
    frames = np.full((B, T), -1, np.int32)
    states = np.full((B, T), -1, np.int32)
    segments = np.full((B, Lmax, 2), -1, np.int32)
    rows = padded.numpy()
    for b in range(B):
        seq = rows[b, :lls[b]].tolist()
        c, path = _band_viterbi(lp[:act[b], b], seq, S, context_order,
                                allow_nonblank_selfloops, eval_repeats_in_context)
        if path is None:
            continue
        cost[b] = c
        states[b, :act[b]] = path
        frames[b, :act[b]] = _band_topology(seq, S, context_order, allow_nonblank_selfloops,
                                            eval_repeats_in_context)[0][path]
        first = np.nonzero(np.r_[True, path[1:] != path[:-1]])[0]
        last = np.r_[first[1:], len(path)]
        odd = path[first] % 2 == 1
        segments[b, path[first][odd] // 2, 0] = first[odd]
        segments[b, path[first][odd] // 2, 1] = last[odd]
    out = [torch.from_numpy(x).to(dev) for x in (cost, frames, states, segments)]
    return CTCAlignment(out[0], out[1], out[2], out[3], torch.isfinite(out[0]))


def alignment_spans(result, labels, label_lens):
    """per utterance, the list of (label, start, end) of a CTCAlignment, in frames"""
    seg = result.segments.cpu().tolist()
    lls = [int(v) for v in torch.as_tensor(label_lens).reshape(-1).tolist()]
    rows = _labels_to_batch(torch.as_tensor(labels).reshape(-1).cpu().long(), lls).tolist()
    feasible = result.feasible.cpu().tolist()
    return [[(rows[b][i], seg[b][i][0], seg[b][i][1]) for i in range(lls[b])] if feasible[b] else []
            for b in range(len(lls))]
