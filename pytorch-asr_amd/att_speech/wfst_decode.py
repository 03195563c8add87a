"""Beam-pruned Viterbi decoding over a weighted finite-state transducer.

The reference scores its systems by writing log-probs (ctc_forward.py) and handing them to
Kaldi's `decode-faster` with the decoding graph CTC_LG_syms.fst, a beam and an acoustic scale
(egs/wsj/ctc_kaldi_decode.sh:141-147).  `decode_graph` is that search: batched, frame-synchronous
token passing over one shared graph, on the device through asr_wfst_decode_f32
(csrc/wfst_decode.hip) and on the host through a numpy path with the same arithmetic.

Semantics (order-independent, so device, host and the tests' fp64 referee
agree bit for bit).  Tropical semiring; arcs (src, ilabel, olabel, weight, dst) in CSR by source,
a source's arcs in the order they were given; "arc index" is the position in that CSR.
ilabel 0 does not consume a frame, ilabel i > 0 reads class i - 1 (decoding_utils/ctc_fst.py:42-44).
The non-emitting arcs must form an acyclic graph.  All arithmetic is fp32, one rounding per step:

1. before frame 0 the start state costs 0; epsilon closure in rank order, c(d) = min(c(d), c(s) + w);
   prune as in 4;
2. frame t: a[i] = -(acoustic_scale * lp[t, b, i - 1]); every survivor s and emitting arc propose
   (c(s) + w) + a[ilabel] to dst; a state's cost is the minimum of its proposals; states above
   the best emitting cost + beam are dropped;
3. epsilon closure over what is left;
4. s survives iff c(s) <= min c + beam (beam = inf: nothing is ever dropped);
5. the last frame is closed but not pruned; the answer is argmin c(s) + final(s) over the final
   states, else (allow_partial) argmin c(s), else nothing (cost +inf).
Equal proposals to one state in one frame, emitting or not: the smallest arc index wins.  Equal
end states: the smallest state id wins.  Proposals that are not finite are ignored.
"""
import os
import warnings

import numpy as np
import torch

from att_speech import _native
from att_speech.lm_fst import LmFst

INF = float('inf')
_NOARC = np.int64(0xFFFFFFFF)
DEFAULT_WORKSPACE_BYTES = 256 << 20


def _ranges(lo, hi):
    """concatenation of arange(lo[i], hi[i]) and the owner index i of every element"""
    n = (hi - lo).astype(np.int64)
    total = int(n.sum())
    owner = np.repeat(np.arange(len(n)), n)
    if total == 0:
        return np.zeros(0, np.int64), owner
    first = np.cumsum(n) - n
    return np.arange(total) - np.repeat(first, n) + np.repeat(lo.astype(np.int64), n), owner


class DecodingGraph(object):
    """A decoding graph as flat arrays: validated, sorted to CSR, epsilon ranks computed, and
    uploaded once per device."""

    def __init__(self, num_states, start, src, dst, ilabel, olabel, weight, final,
                 isymbols=None, osymbols=None):
        n = int(num_states)
        src = np.asarray(src, np.int64).reshape(-1)
        dst = np.asarray(dst, np.int64).reshape(-1)
        il = np.asarray(ilabel, np.int64).reshape(-1)
        ol = np.asarray(olabel, np.int64).reshape(-1)
        w = np.asarray(weight, np.float32).reshape(-1)
        fin = np.asarray(final, np.float32).reshape(-1)
        if not (len(src) == len(dst) == len(il) == len(ol) == len(w)):
            raise ValueError("arc arrays disagree in length")
        if n < 1 or fin.shape != (n,) or not 0 <= int(start) < n:
            raise ValueError("need num_states >= 1, one final cost per state and a start state")
        if n >= 2 ** 31 or len(src) >= 2 ** 32 - 1:
            raise ValueError("graph too large: states must stay below 2^31, arcs below 2^32 - 1")
        if len(src) and (src.min() < 0 or src.max() >= n or dst.min() < 0 or dst.max() >= n):
            raise ValueError("arc end points outside [0, num_states)")
        if len(src) and (il.min() < 0 or il.max() >= 2 ** 31 or np.abs(ol).max() >= 2 ** 31):
            raise ValueError("labels must be non-negative 32-bit integers")
        if not np.isfinite(w).all():
            raise ValueError("arc weights must be finite")
        if np.isnan(fin).any() or (fin == -INF).any():
            raise ValueError("final costs must be finite or +inf")
        order = np.argsort(src, kind='stable')
        self.num_states, self.start = n, int(start)
        self.src, self.dst, self.ilabel, self.olabel, self.weight = (
            src[order], dst[order], il[order], ol[order], w[order])
        self.final = fin
        self.ptr = np.searchsorted(self.src, np.arange(n + 1)).astype(np.int64)
        self.eps_arc = np.nonzero(self.ilabel == 0)[0].astype(np.int64)       # by source: the CSR order
        self.eps_ptr = np.searchsorted(self.src[self.eps_arc], np.arange(n + 1)).astype(np.int64)
        self.rank = self._eps_rank()
        es = self.src[self.eps_arc]
        self.num_ranks = int(self.rank[es].max()) + 1 if len(es) else 0
        self.max_ilabel = int(self.ilabel.max()) if len(src) else 0
        self.isymbols, self.osymbols = isymbols, osymbols
        self._device = {}

    def _eps_rank(self):
        """rank[s]: the length of the longest epsilon path that ends in s (LmFst.eps_rank's
        definition), level by level; ValueError when the epsilon arcs have a cycle."""
        n = self.num_states
        rank = np.zeros(n, np.int64)
        if not len(self.eps_arc):
            return rank
        ed = self.dst[self.eps_arc]
        indeg = np.bincount(ed, minlength=n)
        frontier = np.nonzero(indeg == 0)[0]
        done = 0
        while len(frontier):
            done += len(frontier)
            idx, owner = _ranges(self.eps_ptr[frontier], self.eps_ptr[frontier + 1])
            if not len(idx):
                break
            d = ed[idx]
            np.maximum.at(rank, d, rank[frontier[owner]] + 1)
            indeg -= np.bincount(d, minlength=n)
            d = np.unique(d)
            frontier = d[indeg[d] == 0]
        if (indeg != 0).any():
            raise ValueError("the graph has a cycle of epsilon-input arcs: not decodable frame by frame")
        return rank

    # ---- builders ---------------------------------------------------------------
    @classmethod
    def from_fst(cls, fst):
        """from an LmFst (its arcs are sorted by (source, ilabel); that order is the arc index)"""
        if fst.num_states() < 1 or fst.start() < 0:
            raise ValueError("empty FST")
        return cls(fst.num_states(), fst.start(), fst.src, fst.dst, fst.ilabel, fst.olabel, fst.weight,
                   fst.final_w, fst.input_symbols(), fst.output_symbols())

    @classmethod
    def read(cls, path):
        """an OpenFst binary (vector/standard, plain or gzip) or an AT&T text file"""
        return cls.from_fst(LmFst.read(path))

    @classmethod
    def from_graph_generator(cls, gg):
        """HC (the token transducer of a CTCGraphGen, any context order it builds) or, with a
        grammar, HC o G.  The generator's weights are log-semiring scores: costs are their negation.
        Output labels are the network symbols the HC arcs emit."""
        hc = gg.decoding_fst
        _, out = hc.transition_tables()
        grammar = getattr(gg, 'grammar', None)
        if grammar is None:
            src, dst, il, ol = hc.arcs()
            return cls(hc.num_states, 0, src, dst, np.asarray(il) + 1, ol,
                       np.zeros(len(src), np.float32), np.zeros(hc.num_states, np.float32))
        g = grammar
        live = g.final > 0.5 * gg.nc_weight
        final = np.where(live, -g.final.astype(np.float64), INF)
        ol = out[g.state_pairs[g.src, 0], g.ilabel]
        return cls(g.num_states, 0, g.src, g.dst, np.asarray(g.ilabel) + 1, ol,
                   -g.weight.astype(np.float64), final)

    # ---- device copy ------------------------------------------------------------
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_device'] = {}
        return state

    def device_arrays(self, device):
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        hit = self._device.get(device)
        if hit is None:
            def u32(a):     # uint32 bit patterns in int32 storage
                return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).to(device)

            def pad(a):
                return a if len(a) else np.zeros(1, a.dtype)
            hit = dict(ptr=u32(self.ptr), src=u32(pad(self.src)), dst=u32(pad(self.dst)),
                       il=u32(pad(self.ilabel)), ol=u32(pad(self.olabel.astype(np.int32).view(np.uint32))),
                       w=torch.from_numpy(pad(self.weight)).to(device),
                       fin=torch.from_numpy(self.final).to(device),
                       eps_ptr=u32(self.eps_ptr), eps_arc=u32(pad(self.eps_arc)),
                       rank=u32(self.rank))
            self._device[device] = hit
        return hit


# ----------------------------------------------------------------------------------
# host path: the same proposals, minima and prunes with numpy float32 arithmetic
# ----------------------------------------------------------------------------------
def _merge(g, cost, arcof, act, a, c):
    """proposals (arc a, cost c) into the tables; returns the active list with new states appended"""
    c = c + np.float32(0)                       # -0 and +0 are one cost
    ok = c < INF
    a, c = a[ok], c[ok]
    if not len(a):
        return act
    d = g.dst[a]
    order = np.lexsort((a, c, d))
    a, c, d = a[order], c[order], d[order]
    first = np.nonzero(np.r_[True, d[1:] != d[:-1]])[0]
    a, c, d = a[first], c[first], d[first]
    old_c, old_a = cost[d], arcof[d]
    better = (c < old_c) | ((c == old_c) & (a < old_a))
    new = d[old_c == INF]
    cost[d[better]] = c[better]
    arcof[d[better]] = a[better]
    return np.concatenate([act, new])


def _closure(g, cost, arcof, act):
    for r in range(g.num_ranks):
        s = act[(g.rank[act] == r) & (g.eps_ptr[act + 1] > g.eps_ptr[act])]
        if not len(s):
            continue
        idx, owner = _ranges(g.eps_ptr[s], g.eps_ptr[s + 1])
        a = g.eps_arc[idx]
        act = _merge(g, cost, arcof, act, a, cost[s[owner]] + g.weight[a])
    return act


def _prune(cost, arcof, act, beam):
    if not len(act):
        return act
    c = cost[act]
    keep = c <= c.min() + beam                  # float32 + float32
    drop = act[~keep]
    cost[drop] = INF
    arcof[drop] = _NOARC
    return act[keep]


def _host_one(g, lp, n, beam, scale, allow_partial, cost, arcof):
    """one utterance: lp [T, C] float32.  cost / arcof: dense work tables, all INF / _NOARC on
    entry and on exit.  Returns (words, alignment [T], cost, reached_final, num_active [T], stats)."""
    T = lp.shape[0]
    align = np.full(T, -1, np.int32)
    nact = np.zeros(T, np.int32)
    stats = dict(peak_emit=0, peak_closure=0, records=0, words=0)
    empty = ([], align, np.float32(INF), False, nact, stats)
    if n < 1 or n > T:
        return empty
    beam, scale = np.float32(beam), np.float32(scale)
    cost[g.start], arcof[g.start] = 0.0, _NOARC
    act = np.array([g.start], np.int64)
    frames = []
    cur_s = cur_c = None
    for t in range(-1, n):
        if t >= 0:
            a_sc = -(scale * lp[t])
            arcs, owner = _ranges(g.ptr[cur_s], g.ptr[cur_s + 1])
            em = g.ilabel[arcs] > 0
            arcs, owner = arcs[em], owner[em]
            c = (cur_c[owner] + g.weight[arcs]) + a_sc[g.ilabel[arcs] - 1]
            act = _merge(g, cost, arcof, np.zeros(0, np.int64), arcs, c)
            stats['peak_emit'] = max(stats['peak_emit'], len(act))
            act = _prune(cost, arcof, act, beam)
        act = _closure(g, cost, arcof, act)
        stats['peak_closure'] = max(stats['peak_closure'], len(act))
        stats['records'] += len(act)
        srt = np.sort(act)
        frames.append((srt, arcof[srt].copy()))
        if t < n - 1 and len(act):
            c = cost[act]
            keep = c <= c.min() + beam
            cur_s, cur_c = act[keep], c[keep]
        else:
            cur_s, cur_c = act, cost[act].copy()
        cost[act] = INF
        arcof[act] = _NOARC
        if t >= 0:
            nact[t] = len(cur_s)
    if not len(cur_s):
        return empty
    fin = g.final[cur_s]
    tot = (cur_c + fin) + np.float32(0)
    ok = tot < INF
    reached = bool(ok.any())
    if reached:
        best = tot[ok].min()
        s = int(cur_s[ok][tot[ok] == best].min())
    elif allow_partial:
        best = cur_c.min()
        s = int(cur_s[cur_c == best].min())
    else:
        return empty
    words, k, t = [], n, n - 1
    while True:
        st, ar = frames[k]
        a = int(ar[np.searchsorted(st, s)])
        if a == _NOARC:
            break
        if g.ilabel[a] > 0:
            align[t] = g.ilabel[a]
            t -= 1
            k -= 1
        if g.olabel[a] != 0:
            words.append(int(g.olabel[a]))
        s = int(g.src[a])
    stats['words'] = len(words)
    return words[::-1], align, np.float32(best), reached, nact, stats


def decode_graph_host(lp, lens, graph, beam=16.0, acoustic_scale=1.0, allow_partial=True):
    """The host path on numpy arrays: lp [T,B,C] float32.  Returns the dict of decode_graph with
    numpy fields, plus 'stats': per utterance what a device run needs of its capacities:
    peak_emit / peak_closure (the longest token list after an emitting phase / after a closure,
    against list_cap), records (against log_cap) and words (against word_capacity)."""
    lp = np.asarray(lp, np.float32)
    T, B, _ = lp.shape
    cost = np.full(graph.num_states, INF, np.float32)
    arcof = np.full(graph.num_states, _NOARC, np.int64)
    res = dict(words=[], alignment=np.full((B, T), -1, np.int32), cost=np.full(B, INF, np.float32),
               reached_final=np.zeros(B, bool), num_active=np.zeros((B, T), np.int32),
               redone_on_host=[], stats=[])
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(B):
            w, al, c, rf, na, st = _host_one(graph, lp[:, b], int(lens[b]), beam, acoustic_scale,
                                             allow_partial, cost, arcof)
            res['words'].append(w)
            res['alignment'][b], res['cost'][b], res['reached_final'][b], res['num_active'][b] = al, c, rf, na
            res['stats'].append(st)
    return res


# ----------------------------------------------------------------------------------
# device path
# ----------------------------------------------------------------------------------
def plan_workspace(num_states, T, B, workspace_bytes):
    """(utterances per launch, list_cap, log_cap) for a workspace budget.

    An utterance never needs more than one token per state in a list and one record per state
    and closure in the log: 12 N + 20 N + 8 (T + 1) N bytes.  When the budget holds that for at
    least a quarter of the batch, the batch runs in up to four launches that cannot overflow.
    Otherwise (large graphs, where a beam keeps a small part of the states alive) the per-state
    tables (12 bytes a state and utterance) take at most half of the budget, by splitting the
    batch; a quarter of what is left per utterance goes to the token lists (20 bytes a token),
    the rest to the back-pointer log (8 bytes a record), and an utterance may outgrow them."""
    tables = 12 * num_states
    if workspace_bytes < tables + 20 + 8 + 64:
        raise ValueError("workspace_bytes = %d cannot hold one utterance's tables (%d bytes)"
                         % (workspace_bytes, tables + 92))
    full = tables + (20 + 8 * (T + 1)) * num_states + 64
    if 4 * (workspace_bytes // full) >= B and (T + 1) * num_states < 2 ** 31 - 1:
        return int(min(B, workspace_bytes // full)), int(num_states), int((T + 1) * num_states)
    chunk = B if B * tables <= workspace_bytes // 2 else max(1, (workspace_bytes // 2) // tables)
    # every utterance of a launch needs its tables, one list slot and one record
    chunk = max(1, min(chunk, B, workspace_bytes // (tables + 20 + 8 + 64)))
    rest = workspace_bytes // chunk - tables - 64
    list_cap = int(min(num_states, max(1, rest // 4 // 20), 2 ** 31 - 2))
    log_cap = int(min((T + 1) * list_cap, max(1, (rest - 20 * list_cap) // 8), 2 ** 31 - 2))
    return chunk, list_cap, log_cap


def word_capacity(T, num_ranks):
    """output labels a path may carry on the device: one per arc, up to eight arcs a frame"""
    return (T + 1) * min(num_ranks + 1, 8)


# threads per workgroup handed to asr_wfst_decode_f32: 0 = its measured default; 256 / 512 / 1024 are
# set by tools/bench_wfst_decode.py --sweep-threads and by nothing else
THREADS_PER_WORKGROUP = 0


def _decode_device(lp, lens, graph, beam, scale, allow_partial, workspace_bytes):
    T, B, C = lp.shape
    L = _native.lib()
    g = graph
    if not L.asr_wfst_decode_supported(g.num_states, len(g.src), C, T):
        raise NotImplementedError(
            "asr_wfst_decode_f32 serves 1 <= C <= 4096 classes and T >= 1 (got C = %d, T = %d); "
            "ASR_WFST_NATIVE=0 selects the host path" % (C, T))
    dev = lp.device
    d = g.device_arrays(dev)
    lens_d = torch.as_tensor(np.asarray(lens, np.int32)).to(dev)
    chunk, list_cap, log_cap = plan_workspace(g.num_states, T, B, workspace_bytes)
    word_cap = word_capacity(T, g.num_ranks)
    i32 = dict(dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.float32, device=dev)
    final, nwords, overflow = (torch.empty(B, **i32) for _ in range(3))
    align, nact = torch.empty((B, T), **i32), torch.empty((B, T), **i32)
    words = torch.empty((B, word_cap), **i32)
    nbytes = L.asr_wfst_decode_workspace_bytes(g.num_states, chunk, list_cap, log_cap)
    if not 0 < nbytes <= workspace_bytes:
        raise ValueError("workspace_bytes = %d is too small: %d utterances a launch with %d list slots and "
                         "%d records need %d bytes" % (workspace_bytes, chunk, list_cap, log_cap, nbytes))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = _native._p
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        _native.check(L.asr_wfst_decode_f32(
            p(lp[:, b0]), B * C, p(lens_d[b0:]), T, b1 - b0, C, g.num_states, len(g.src),
            p(d['ptr']), p(d['src']), p(d['dst']), p(d['il']), p(d['ol']), p(d['w']), p(d['fin']),
            p(d['eps_ptr']), p(d['eps_arc']), len(g.eps_arc), p(d['rank']), g.num_ranks, g.start,
            float(beam), float(scale), int(bool(allow_partial)), list_cap, log_cap, word_cap,
            int(THREADS_PER_WORKGROUP),
            p(cost[b0:]), p(final[b0:]), p(align[b0:]), p(nact[b0:]), p(words[b0:]), p(nwords[b0:]),
            p(overflow[b0:]), p(ws), nbytes, _native._stream()), 'asr_wfst_decode_f32')
    return cost, final, align, nact, words, nwords, overflow


def decode_graph(log_probs, lens, graph, beam=16.0, acoustic_scale=1.0, allow_partial=True,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """Best path of every utterance through `graph` under a beam.

    log_probs [T,B,C] float32 (any per-frame scores; costs are their negation times
    acoustic_scale), lens [B] frames per utterance (>= 1), graph a DecodingGraph.
    Returns a dict: words (list of lists: the olabels != 0 along the path), alignment [B,T] int32
    (the ilabel of each frame's emitting arc, -1 beyond lens), cost [B] float32 (+inf and empty
    fields when there is no result), reached_final [B] bool, num_active [B,T] int32 (tokens
    surviving each frame's last prune; the last frame is not pruned), redone_on_host (indices).

    A GPU tensor runs asr_wfst_decode_f32; a CPU tensor, or ASR_WFST_NATIVE=0 (read per call), the
    host path, which gives the same bits.  workspace_bytes bounds the device workspace
    (plan_workspace): a batch whose tables exceed it runs in several launches, and an utterance
    that outgrows its token lists or its log is redone on the host, with one warning per call."""
    if not isinstance(log_probs, torch.Tensor):
        log_probs = torch.as_tensor(np.asarray(log_probs, np.float32))
    if log_probs.dim() != 3:
        raise ValueError("log_probs must be [T, B, C]")
    T, B, C = log_probs.shape
    if graph.max_ilabel > C:
        raise ValueError("the graph reads class %d but log_probs has C = %d classes"
                         % (graph.max_ilabel - 1, C))
    if not (float(beam) >= 0.0):
        raise ValueError("beam must be >= 0")
    lens_np = np.asarray(torch.as_tensor(lens).cpu(), np.int64).reshape(-1)
    if len(lens_np) != B:
        raise ValueError("lens must have one entry per utterance")
    if len(lens_np) and (lens_np.min() < 1 or lens_np.max() > T):
        raise ValueError("lens must lie in [1, T]")
    lp = log_probs.detach()
    if lp.dtype != torch.float32:
        lp = lp.float()
    native = lp.is_cuda and os.environ.get('ASR_WFST_NATIVE', '1') != '0'
    if not native or B == 0 or T == 0:
        res = decode_graph_host(lp.cpu().numpy(), lens_np, graph, beam, acoustic_scale, allow_partial)
        res.pop('stats')
        for k in ('alignment', 'cost', 'reached_final', 'num_active'):
            res[k] = torch.from_numpy(res[k]).to(log_probs.device)
        return res
    lp = lp.contiguous()
    cost, final, align, nact, words, nwords, overflow = _decode_device(
        lp, lens_np, graph, beam, acoustic_scale, allow_partial, int(workspace_bytes))
    nw = nwords.cpu().numpy()
    wd = words.cpu().numpy()
    redo = np.nonzero(overflow.cpu().numpy())[0].tolist()
    out_words = [wd[b, :nw[b]][::-1].tolist() for b in range(B)]
    final = final != 0
    if redo:
        warnings.warn("decode_graph: %d of %d utterances outgrew the device workspace "
                      "(workspace_bytes = %d) and were decoded on the host"
                      % (len(redo), B, workspace_bytes))
        idx = torch.as_tensor(redo, device=lp.device)
        h = decode_graph_host(lp[:, idx].cpu().numpy(), lens_np[redo], graph, beam, acoustic_scale,
                              allow_partial)
        for j, b in enumerate(redo):
            out_words[b] = h['words'][j]
        align[idx] = torch.from_numpy(h['alignment']).to(lp.device)
        nact[idx] = torch.from_numpy(h['num_active']).to(lp.device)
        cost[idx] = torch.from_numpy(h['cost']).to(lp.device)
        final[idx] = torch.from_numpy(h['reached_final']).to(lp.device)
    return dict(words=out_words, alignment=align, cost=cost, reached_final=final, num_active=nact,
                redone_on_host=redo)
