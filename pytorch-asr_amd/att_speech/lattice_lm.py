"""Rescoring lattices with a back-off n-gram language model: lattice o G, on the device.

The recipes decode with a small LM compiled into the graph and rescore the lattice with a larger one
(Kaldi's lattice-lmrescore between latgen-faster and lattice-best-path).  `rescore_lm` composes every
lattice of a batch with an LM and returns another batch of the same kind over a graph of its own, so
best_paths, nbest, sentences, posteriors and mbr run on the result unchanged.  DESIGN.md section 4.24.

The LM in back-off form (`BackoffLm.from_fst`, derived on the host in fp64 from an LmFst acceptor):

  * an epsilon arc whose destination has no outgoing arcs is a sentence-end arc and folds into the
    final cost of its source: final0(q) = min(final(q), w + final(dst));
  * of the remaining epsilon arcs a state has at most one, its back-off arc (two: ValueError); two
    non-epsilon arcs with one label out of one state and a cycle of back-off arcs are ValueErrors;
  * step(q, l): c = 0; if q has an arc labelled l, return (dst, c + w); else if q has a back-off arc,
    c += w_bo, q = its destination, repeat; else there is no match.  fp64 sums in exactly this order;
  * final*(q) = final0(q) where that is finite, else w_bo + final*(backoff(q)); +inf at the end of
    the chain.

This is the ARPA reading of a back-off model (Kaldi's BackoffDeterministicOnDemandFst): deterministic, so
a lattice path maps to at most one rescored path, and path counts, posteriors and MBR masses stay honest.

The composition.  A node of the result is (lattice node v, LM state q).  The nodes of time 0 whose graph
state is graph.start are seeded with lm.start().  A lattice arc j: u -> v without a word carries q
unchanged at LM cost 0; one with word o looks up l = label_map[o] and goes to step(q, l).  label_map[o] <= 0
(or o outside the map) and "no match" are out of vocabulary: the arc costs oov_cost and leaves q where the
chain ended; oov_cost = inf drops it.

The result's graph (`RescoredGraph`, a DecodingGraph) is the part of graph o LM the batch visited: states
are the distinct (graph state, LM state) pairs of the kept nodes of the whole call plus the start pair, in
sorted order; arcs the distinct (graph arc a, q) pairs of the kept arcs by (source id, a), with the labels
of a, weight = float32(float64(w[a]) + scale * c) and final = float32(float64(final[s]) + scale * final*(q))
(+inf if either term is infinite).  base, lm, state_pairs and arc_base project back.

alpha, beta and the pruning, in fp32 with one rounding per operation (DESIGN.md section 4.20 with the new
weights w'; a = -(float32(acoustic scale) * lp), the utterance's own scale):

  alpha(seed) = 0, alpha(v) = min over arcs u -> v of ((alpha(u) + w') + a) + 0
  beta(v) = end(v) for the end nodes (final' of its pair; 0 on every node of the last time of a partial
  lattice), beta(u) = min(beta(u), ((w' + a) + beta(v)) + 0)
  best = min over the end nodes of (alpha + end) + 0: the utterance's new cost
  kept: alpha(u) + (((w' + a) + beta(v)) + 0) is finite and <= best + lattice_beam (None: finite), plus
  the arcs of the forward traceback from the first end node that attains best (per node the first in-arc
  in (source, graph arc) order that attains alpha), so that lattice_beam = 0 keeps a best path whatever
  the rounding; kept nodes are the end points of kept arcs.  No kept arc: the empty lattice, cost +inf.

Minima do not depend on the schedule, so the device path (asr_lattice_lmrescore_* of csrc/lattice_lm.hip)
and the numpy twin below agree bit for bit.  scale = -1 with the first-pass LM followed by scale = 1 with
the new one is the recipe's "take the old LM out, put the new one in"; the first-pass graph treated
epsilons as ordinary arcs (the search may have taken a back-off arc although the n-gram existed), so taking
its LM out under the back-off reading is the usual approximation, as in Kaldi's recipe.
"""
import ctypes
import warnings

import numpy as np
import torch

from att_speech import _native
from att_speech.lm_fst import LmFst
from att_speech.wfst_decode import DecodingGraph, _ranges
from att_speech.wfst_lattice import INF, Lattice

DEFAULT_MAX_LM_STATES = 256     # LM states a lattice node may hold on the device (a run-time argument)
DEVICE_MAX_LM_STATES = 1024     # ASR_LATTICE_LMRESCORE_MAX_STATES: a wave's list under construction sits in LDS
THREADS_PER_WORKGROUP = 256


class BackoffLm(object):
    """An LmFst acceptor in back-off form (the module docstring states the rules)."""

    def __init__(self, fst):
        self.fst = fst
        n = self.num_states = fst.num_states()
        if n < 1 or fst.start() < 0:
            raise ValueError("empty LM")
        eps = fst.ilabel == 0
        out_deg = np.diff(fst.ptr)
        is_end = eps & (out_deg[fst.dst] == 0) if len(eps) else eps
        final0 = fst.final_w.astype(np.float64).copy()
        np.minimum.at(final0, fst.src[is_end], fst.weight[is_end] + fst.final_w[fst.dst[is_end]])
        bo = eps & ~is_end
        if len(bo) and (np.bincount(fst.src[bo], minlength=n) > 1).any():
            raise ValueError("an LM state has two back-off arcs: not a back-off model")
        ne = ~eps
        src, lab = fst.src[ne], fst.ilabel[ne]
        if len(src) > 1 and ((src[1:] == src[:-1]) & (lab[1:] == lab[:-1])).any():
            raise ValueError("two arcs with one label leave one LM state: not deterministic")
        rank = fst.eps_rank()
        if rank is None:
            raise ValueError("the back-off arcs of the LM form a cycle")
        self.final0 = final0
        self.bo_dst = np.full(n, -1, np.int64)
        self.bo_w = np.zeros(n, np.float64)
        self.bo_dst[fst.src[bo]] = fst.dst[bo]
        self.bo_w[fst.src[bo]] = fst.weight[bo]
        self.ptr = np.searchsorted(src, np.arange(n + 1)).astype(np.int64)
        self.label, self.dst, self.weight = lab.astype(np.int64), fst.dst[ne].astype(np.int64), fst.weight[ne]
        self.num_labels = int(lab.max()) + 1 if len(lab) else 1
        self._key = src * self.num_labels + self.label
        self.max_chain = int(rank.max()) if n else 0
        fs = final0.copy()
        for r in range(self.max_chain, -1, -1):           # a back-off arc leads to a higher epsilon rank
            s = np.nonzero((rank == r) & ~(final0 < INF) & (self.bo_dst >= 0))[0]
            fs[s] = self.bo_w[s] + fs[self.bo_dst[s]]
        self.final_star_all = fs
        self._device = {}

    @classmethod
    def from_fst(cls, lm):
        """lm: a BackoffLm (returned as it is), an LmFst, or whatever LmFst.read takes"""
        if isinstance(lm, cls):
            return lm
        if not isinstance(lm, LmFst):
            lm = LmFst.read(lm)
        return cls(lm)

    def start(self):
        return self.fst.start()

    def input_symbols(self):
        return self.fst.input_symbols()

    def step_many(self, q, l):
        """step for arrays: (state where the chain ended or the match led, cost, matched)"""
        q = np.asarray(q, np.int64).copy()
        l = np.asarray(l, np.int64)
        c = np.zeros(len(q), np.float64)
        matched = np.zeros(len(q), bool)
        live = l > 0
        valid = l < self.num_labels
        for _ in range(self.max_chain + 1):
            idx = np.nonzero(live)[0]
            if not len(idx):
                break
            hit = np.zeros(len(idx), bool)
            if len(self._key):
                k = q[idx] * self.num_labels + np.where(valid[idx], l[idx], 0)
                pos = np.minimum(np.searchsorted(self._key, k), len(self._key) - 1)
                hit = (self._key[pos] == k) & valid[idx]
                h, ph = idx[hit], pos[hit]
                c[h] = c[h] + self.weight[ph]
                q[h] = self.dst[ph]
                matched[h] = True
                live[h] = False
            m = idx[~hit]
            bo = self.bo_dst[q[m]]
            live[m[bo < 0]] = False
            mm = m[bo >= 0]
            c[mm] = c[mm] + self.bo_w[q[mm]]
            q[mm] = bo[bo >= 0]
        return q, c, matched

    def step(self, q, l):
        """(next state, cost) or None when nothing along the back-off chain matches"""
        qo, c, ok = self.step_many([q], [l])
        return (int(qo[0]), float(c[0])) if ok[0] else None

    def final_star(self, q):
        return float(self.final_star_all[q])

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
            if self.num_states >= 2 ** 31 - 1 or len(self.label) >= 2 ** 31 - 1 or self.num_labels >= 2 ** 31 - 1:
                raise NotImplementedError("the LM is too large for the device path")

            def up(a, dtype):
                a = np.ascontiguousarray(a, dtype)
                return torch.from_numpy(a if len(a) else np.zeros(1, dtype)).to(device)
            hit = dict(ptr=up(self.ptr, np.int32), label=up(self.label, np.int32), dst=up(self.dst, np.int32),
                       weight=up(self.weight, np.float64), bo_dst=up(self.bo_dst, np.int32),
                       bo_w=up(self.bo_w, np.float64), final_star=up(self.final_star_all, np.float64))
            self._device[device] = hit
        return hit


def lm_label_map(lm, vocabulary, num_symbols):
    """label_map for graphs built by DecodingGraph.from_graph_generator, whose output labels are network
    symbols: the inverse of fst_utils.grammar_labels.  [num_symbols] int64, entry o the LM's label of
    network symbol o, -1 where the LM has none; 0 maps to 0."""
    from att_speech.fst_utils import _read_vocabulary, grammar_labels
    fst = lm.fst if isinstance(lm, BackoffLm) else lm
    net = grammar_labels(fst, _read_vocabulary(vocabulary) if vocabulary is not None else None, num_symbols)
    out = np.full(int(num_symbols), -1, np.int64)
    for k in range(len(net) - 1, 0, -1):                # of two LM labels with one network symbol the smaller
        if 0 < net[k] < num_symbols:
            out[net[k]] = k
    out[0] = 0
    return out


def _default_label_map(graph, blm):
    top = int(np.abs(graph.olabel).max()) + 1 if len(graph.olabel) else 1
    gs, ls = graph.osymbols, blm.input_symbols()
    if gs is None or ls is None:
        return np.arange(top, dtype=np.int64)
    out = np.full(top, -1, np.int64)
    for k, sym in gs:
        if 0 < k < top:
            out[k] = ls.find(sym)
    out[0] = 0
    return out


class RescoredGraph(DecodingGraph):
    """The part of graph o LM that one rescore_lm call visited.  base: the graph the lattices came with;
    lm: the BackoffLm; scale; state_pairs [n, 2]: (base state, LM state) of every state, sorted; arc_base
    [m]: the base arc of every arc; arc_lm_state, arc_lm_cost [m]: the LM state at the arc's source and
    the LM cost c that went into its weight."""

    def __init__(self, base, lm, scale, state_pairs, src, dst, arc_base, arc_lm_state, arc_lm_cost):
        pairs = np.asarray(state_pairs, np.int64).reshape(-1, 2)
        arc_base = np.asarray(arc_base, np.int64)
        c = np.asarray(arc_lm_cost, np.float64)
        scale = float(scale)
        weight = (base.weight[arc_base].astype(np.float64) + scale * c).astype(np.float32)
        f_g = base.final[pairs[:, 0]].astype(np.float64)
        f_l = lm.final_star_all[pairs[:, 1]]
        ok = (f_g < INF) & (f_l < INF)
        with np.errstate(invalid='ignore', over='ignore'):
            final = np.where(ok, (f_g + scale * np.where(ok, f_l, 0.0)).astype(np.float32), np.float32(INF))
        start = int(np.searchsorted(pairs[:, 0] * lm.num_states + pairs[:, 1],
                                    base.start * lm.num_states + lm.start()))
        DecodingGraph.__init__(self, len(pairs), start, src, dst, base.ilabel[arc_base], base.olabel[arc_base],
                               weight, final, base.isymbols, base.osymbols)
        self.base, self.lm, self.scale = base, lm, scale
        self.state_pairs, self.arc_base = pairs, arc_base
        self.arc_lm_state, self.arc_lm_cost = np.asarray(arc_lm_state, np.int64), c


# ----------------------------------------------------------------------------------
# the numpy twin: expansion level by level, then the two sweeps
# ----------------------------------------------------------------------------------
class _View(object):
    """the lattices of a batch laid end to end on the host"""

    def __init__(self, lats, graph):
        self.graph = g = graph
        nn = np.array([l.num_nodes for l in lats], np.int64)
        na = np.array([l.num_arcs for l in lats], np.int64)
        self.B = len(lats)
        self.node_off, self.arc_off = np.r_[0, np.cumsum(nn)].astype(np.int64), np.r_[0, np.cumsum(na)].astype(np.int64)
        self.node_utt = np.repeat(np.arange(self.B), nn)
        a_utt = np.repeat(np.arange(self.B), na)

        def cat(name, dtype):
            parts = [np.asarray(getattr(l, name), dtype) for l in lats]
            return np.concatenate(parts) if parts else np.zeros(0, dtype)
        self.time, self.state = cat('time', np.int64), cat('state', np.int64)
        self.src = cat('src', np.int64) + self.node_off[a_utt]
        self.dst = cat('dst', np.int64) + self.node_off[a_utt]
        self.arc, self.lp = cat('arc', np.int64), cat('lp', np.float32)
        self.frames = np.array([l.num_frames for l in lats], np.int64)
        self.reached = np.array([l.reached_final for l in lats], bool)
        self.scale = np.array([l.acoustic_scale for l in lats], np.float64)
        self.cost = np.array([l.cost for l in lats], np.float32)
        R = g.num_ranks + 1
        t_max = int(self.time.max()) + 1 if len(self.time) else 1
        key = (self.node_utt * t_max + self.time) * R + g.rank[self.state] if len(self.time) else self.time
        _, self.level = np.unique(key, return_inverse=True)        # the level index of every node, ascending


def _groups(key):
    """index groups of equal key, by ascending key"""
    order = np.argsort(key, kind='stable')
    if not len(order):
        return []
    k = key[order]
    cuts = np.nonzero(np.r_[True, k[1:] != k[:-1]])[0]
    return [(int(k[a]), order[a:b]) for a, b in zip(cuts, list(cuts[1:]) + [len(order)])]


def _twin_piece(view, select, blm, lmap, scale, lattice_beam, oov_cost):
    """Expansion, sweeps and pruning of the selected utterances on the host.  Returns (piece, best [B]
    float32, stats): piece holds the kept nodes (n_v: batch node, n_q, alpha, beta) by (n_v, n_q) and the kept
    arcs (src, dst: indices into the piece's nodes; j: batch arc; q, c) by (src, j)."""
    g, N, Q = view.graph, len(view.time), blm.num_states
    f32, zero = np.float32, np.float32(0)
    ol = g.olabel[view.arc] if len(view.arc) else np.zeros(0, np.int64)
    out_ptr = np.searchsorted(view.src, np.arange(N + 1))
    seeds = np.nonzero((view.time == 0) & (view.state == g.start) & select[view.node_utt])[0] if N else np.zeros(0, np.int64)
    pend = {}
    for lv, idx in _groups(view.level[seeds]):
        pend.setdefault(lv, []).append((seeds[idx], np.full(len(idx), blm.start(), np.int64)))
    n_v, n_q, parts = [], [], []
    stats = dict(max_lm_states=0, dropped_arcs=0)
    for lv in range(int(view.level.max()) + 1 if N else 0):
        if lv not in pend:
            continue
        key = np.unique(np.concatenate([v * Q + q for v, q in pend.pop(lv)]))
        pv, pq = key // Q, key % Q
        stats['max_lm_states'] = max(stats['max_lm_states'], int(np.unique(pv, return_counts=True)[1].max()))
        n_v.append(pv), n_q.append(pq)
        js, owner = _ranges(out_ptr[pv], out_ptr[pv + 1])
        if not len(js):
            continue
        qu, o = pq[owner], ol[js]
        word = o != 0
        inside = (o > 0) & (o < len(lmap))
        l = np.where(inside, lmap[np.where(inside, o, 0)], -1)
        qd, c, ok = qu.copy(), np.zeros(len(js)), np.ones(len(js), bool)
        sq, sc, matched = blm.step_many(qu[word], l[word])
        qd[word], c[word] = sq, np.where(matched, sc, oov_cost)
        ok[word] = matched | (oov_cost < INF)
        stats['dropped_arcs'] += int((~ok).sum())
        u, qu, js, qd, c = pv[owner][ok], qu[ok], js[ok], qd[ok], c[ok]
        vd = view.dst[js]
        parts.append((u, qu, js, vd, qd, c))
        for lv2, idx in _groups(view.level[vd]):
            pend.setdefault(lv2, []).append((vd[idx], qd[idx]))
    best = np.full(view.B, INF, np.float32)
    empty = dict(n_v=np.zeros(0, np.int64), n_q=np.zeros(0, np.int64), alpha=np.zeros(0, f32), beta=np.zeros(0, f32),
                 src=np.zeros(0, np.int64), dst=np.zeros(0, np.int64), j=np.zeros(0, np.int64),
                 q=np.zeros(0, np.int64), c=np.zeros(0, np.float64))
    if not n_v:
        return empty, best, stats
    nkey = np.sort(np.concatenate(n_v) * Q + np.concatenate(n_q))
    NV, NQ = nkey // Q, nkey % Q
    E = len(nkey)
    if parts:
        u, qu, js, vd, qd, c = (np.concatenate(x) for x in zip(*parts))
    else:
        u = qu = js = vd = qd = np.zeros(0, np.int64)
        c = np.zeros(0)
    src, dst = np.searchsorted(nkey, u * Q + qu), np.searchsorted(nkey, vd * Q + qd)
    order = np.lexsort((js, src))
    src, dst, js, qu, c = src[order], dst[order], js[order], qu[order], c[order]
    # ---- the sweeps
    utt = view.node_utt[NV]
    a_utt = utt[src]
    with np.errstate(invalid='ignore', over='ignore'):
        w1 = (g.weight[view.arc[js]].astype(np.float64) + float(scale) * c).astype(f32)
        ac = -(view.scale[a_utt].astype(f32) * view.lp[js])
        f_g, f_l = g.final[view.state[NV]].astype(np.float64), blm.final_star_all[NQ]
        fin = (f_g < INF) & (f_l < INF)
        end = np.where(fin, (f_g + float(scale) * np.where(fin, f_l, 0.0)).astype(f32), f32(INF))
        end = np.where(view.time[NV] == view.frames[utt], np.where(view.reached[utt], end, zero), f32(INF)).astype(f32)
        alpha = np.full(E, INF, f32)
        is_seed = (view.time[NV] == 0) & (view.state[NV] == g.start) & (NQ == blm.start())
        alpha[is_seed] = 0
        elevel = view.level[NV]
        groups = _groups(elevel[src])
        for _, idx in groups:
            cand = ((alpha[src[idx]] + w1[idx]) + ac[idx]) + zero
            m = cand < INF
            np.minimum.at(alpha, dst[idx][m], cand[m])
        beta = (end + zero).astype(f32)
        for _, idx in reversed(groups):
            qv = ((w1[idx] + ac[idx]) + beta[dst[idx]]) + zero
            m = qv < INF
            np.minimum.at(beta, src[idx][m], qv[m])
        tot = (alpha + end) + zero
        m = tot < INF
        np.minimum.at(best, utt[m], tot[m])
        # the forward traceback from the first end node that attains best
        at = np.nonzero(m & (tot == best[utt]))[0]
        endnode = np.full(view.B, E, np.int64)
        np.minimum.at(endnode, utt[at], at)
        cand = ((alpha[src] + w1) + ac) + zero
        win = np.nonzero((cand == alpha[dst]) & (cand < INF))[0]
        bp = np.full(E, len(src), np.int64)
        np.minimum.at(bp, dst[win], win)
        bp[is_seed] = len(src)
        forced = np.zeros(len(src), bool)
        cur = endnode[endnode < E]
        while len(cur):
            j = bp[cur]
            j = j[j < len(src)]
            forced[j] = True
            cur = src[j]
        qv = ((w1 + ac) + beta[dst]) + zero
        val = alpha[src] + qv
        limit = best + f32(lattice_beam) if lattice_beam is not None else np.full(view.B, INF, f32)
        keep = ((val < INF) & (val <= limit[a_utt])) | forced
    used = np.zeros(E, bool)
    used[src[keep]] = True
    used[dst[keep]] = True
    new_id = np.cumsum(used) - 1
    live = np.zeros(view.B, bool)
    live[utt[used]] = True
    best = np.where(live, best, f32(INF)).astype(f32)
    piece = dict(n_v=NV[used], n_q=NQ[used], alpha=alpha[used], beta=beta[used], src=new_id[src[keep]],
                 dst=new_id[dst[keep]], j=js[keep], q=qu[keep], c=c[keep])
    return piece, best, stats


# ----------------------------------------------------------------------------------
# the device path: asr_lattice_lmrescore_expand / _emit / _sweep
# ----------------------------------------------------------------------------------
def _device_piece(batch, blm, lmap, scale, lattice_beam, oov_cost, cap, budget):
    """_twin_piece on the device, for the utterances that fit max_lm_states = cap: (piece of tensors, best [B]
    tensor, stats, the utterances that outgrew the cap)"""
    L = _native.lib()
    dev, p = batch.device, _native._p
    B, N, A = batch.num_utterances, batch.num_nodes, batch.num_arcs
    g = batch.graph.device_arrays(dev)
    lm = blm.device_arrays(dev)
    lmap_d = torch.from_numpy(np.ascontiguousarray(lmap, np.int64)).to(dev)
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    cnt = torch.zeros(N, **i32)
    status = torch.zeros(B, **i32)
    G, S, Q = len(batch.graph.src), batch.graph.num_states, blm.num_states
    lm_args = (Q, len(blm.label), p(lm['ptr']), p(lm['label']), p(lm['dst']), p(lm['weight']), p(lm['bo_dst']),
               p(lm['bo_w']), blm.start(), p(lmap_d), len(lmap), float(oov_cost))
    chunks = batch._utterance_chunks(4 * cap, budget - 64)
    out = {k: [] for k in ('n_v', 'n_q', 'src', 'dst', 'j', 'q', 'c', 'w', 'a')}
    e_base = 0
    dropped = 0
    batch.launches = 0
    for b0, b1 in chunks:
        n0, n1 = int(batch.node_off[b0]), int(batch.node_off[b1])
        a0, a1 = int(batch.arc_off[b0]), int(batch.arc_off[b1])
        if n1 == n0:
            continue
        nbytes = L.asr_lattice_lmrescore_workspace_bytes(n1 - n0, cap)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        batch._check(L.asr_lattice_lmrescore_expand(
            B, b0, b1 - b0, cap, N, A, batch.num_levels, _h64(batch.node_off), p(batch.node_off_d),
            p(batch.level_off_d), p(batch.time), p(batch.state), p(batch.src_global), p(batch.arc),
            p(batch.level_ptr), p(batch.level_node), p(batch.in_ptr), p(batch.in_arc), G, p(g['ol']), batch.graph.start,
            *lm_args, p(cnt), p(status), p(ws), nbytes, _native._stream()),
            'asr_lattice_lmrescore_expand')
        batch.launches += 1
        ok_node = status[batch.node_utt[n0:n1]] == 0
        c = torch.where(ok_node, cnt[n0:n1], torch.zeros_like(cnt[n0:n1]))
        cnt[n0:n1] = c
        c = c.long()
        e_off = torch.cat([torch.zeros(1, **i64), torch.cumsum(c, 0)])
        per_arc = c[batch.src_global[a0:a1] - n0]
        slot = torch.cat([torch.zeros(1, **i64), torch.cumsum(per_arc, 0)])
        E, M = int(e_off[-1]), int(slot[-1])
        if max(E, M) >= 2 ** 31 - 1:
            raise NotImplementedError("rescore_lm: more than 2^31 - 1 nodes or arcs in one launch; lower "
                                      "workspace_bytes or prune the lattices")
        if E == 0:
            continue
        n_q = torch.empty(E, **i32)
        e_src, e_dst, e_q, e_ok = (torch.zeros(max(M, 1), **i32) for _ in range(4))
        e_c = torch.zeros(max(M, 1), dtype=torch.float64, device=dev)
        e_w, e_a = (torch.zeros(max(M, 1), dtype=torch.float32, device=dev) for _ in range(2))
        batch._check(L.asr_lattice_lmrescore_emit(
            B, b0, b1 - b0, cap, N, A, _h64(batch.node_off), _h64(batch.arc_off), p(batch.src_global),
            p(batch.dst_global), p(batch.arc_utt), p(batch.arc), p(batch.lp), p(batch.scale_d), G, p(g['ol']), p(g['w']),
            *lm_args, float(scale), p(cnt), p(e_off), p(slot), E, M, p(n_q), p(e_src),
            p(e_dst), p(e_q), p(e_c), p(e_w), p(e_a), p(e_ok), p(ws), nbytes, _native._stream()),
            'asr_lattice_lmrescore_emit')
        batch.launches += 1
        okm = e_ok[:M] == 1
        if bool((e_ok[:M] < 0).any()):
            raise ValueError("asr_lattice_lmrescore_emit: the batch's index arrays are inconsistent")
        e_j = torch.repeat_interleave(torch.arange(a0, a1, **i64), per_arc, output_size=M)
        keep = torch.nonzero(okm).reshape(-1)
        dropped += M - int(keep.numel())
        srt = torch.sort(e_src[:M][keep].long(), stable=True)[1]
        keep = keep[srt]
        out['n_v'].append(torch.repeat_interleave(torch.arange(n0, n1, **i64), c, output_size=E))
        out['n_q'].append(n_q.long())
        out['src'].append(e_src[:M][keep].long() + e_base), out['dst'].append(e_dst[:M][keep].long() + e_base)
        out['j'].append(e_j[keep]), out['q'].append(e_q[:M][keep].long()), out['c'].append(e_c[:M][keep])
        out['w'].append(e_w[:M][keep]), out['a'].append(e_a[:M][keep])
        e_base += E
    status_h = status.cpu().numpy()
    if (status_h & 2).any():
        raise ValueError("asr_lattice_lmrescore_expand: the batch's index arrays are inconsistent")
    redo = np.nonzero(status_h & 1)[0].tolist()
    stats = dict(max_lm_states=int(cnt.max()) if N else 0, dropped_arcs=dropped)
    f32 = dict(dtype=torch.float32, device=dev)
    best = torch.full((B,), INF, **f32)
    if not out['n_v']:
        z, zf = torch.zeros(0, **i64), torch.zeros(0, **f32)
        return dict(n_v=z, n_q=z, alpha=zf, beta=zf, src=z, dst=z, j=z, q=z,
                    c=torch.zeros(0, dtype=torch.float64, device=dev)), best, stats, redo
    u = {k: torch.cat(v) for k, v in out.items()}
    n_v, n_q, src, dst = u['n_v'], u['n_q'], u['src'], u['dst']
    E, M = int(n_v.numel()), int(src.numel())
    # the level structure of the expanded lattice: a node (v, q) sits at v's level
    n_utt = batch.node_utt[n_v]
    lev = batch.node_level.long()[n_v]
    perm = torch.sort(lev, stable=True)[1]
    ck = lev[perm]
    new = torch.ones(E, dtype=torch.bool, device=dev)
    new[1:] = ck[1:] != ck[:-1]
    first = torch.nonzero(new).reshape(-1)
    EL = int(first.numel())
    level_ptr = torch.cat([first, torch.full((1,), E, **i64)]).int()
    ends_b = torch.arange(B + 1, **i64)
    level_off = torch.searchsorted(n_utt[perm][first].contiguous(), ends_b)
    node_off = torch.searchsorted(n_utt.contiguous(), ends_b)
    arc_off = torch.searchsorted(n_utt[src].contiguous(), ends_b) if M else torch.zeros(B + 1, **i64)
    ends = torch.arange(E + 1, **i64)
    order = torch.sort(dst, stable=True)[1] if M else dst
    in_ptr = torch.searchsorted(dst[order].contiguous(), ends).int()
    out_ptr = torch.searchsorted(src.contiguous(), ends).int()
    alpha, beta = torch.full((E,), INF, **f32), torch.full((E,), INF, **f32)
    keep = torch.zeros(max(M, 1), **i32)
    st = torch.zeros(B, **i32)
    src32, dst32 = src.int(), dst.int()
    n_v32, n_q32, order32, perm32 = n_v.int(), n_q.int(), order.int(), perm.int()
    beam = INF if lattice_beam is None else float(lattice_beam)
    batch._check(L.asr_lattice_lmrescore_sweep(
        B, E, M, EL, N, p(node_off), p(arc_off), p(level_off), p(level_ptr), p(perm32), p(in_ptr), p(order32),
        p(out_ptr), p(src32), p(dst32), p(u['w']), p(u['a']), p(n_v32), p(n_q32), p(batch.time), p(batch.state),
        p(batch.frames_d), p(batch.reached_d), S, p(g['fin']), batch.graph.start, Q, p(lm['final_star']), blm.start(),
        float(scale), beam, int(THREADS_PER_WORKGROUP), p(alpha), p(beta), p(keep), p(best), p(st),
        _native._stream()), 'asr_lattice_lmrescore_sweep')
    batch.launches += 1
    if bool(st.any()):
        raise ValueError("asr_lattice_lmrescore_sweep: the expanded lattice's index arrays are inconsistent")
    kept = torch.nonzero(keep[:M] == 1).reshape(-1)
    used = torch.zeros(E, dtype=torch.bool, device=dev)
    used[src[kept]] = True
    used[dst[kept]] = True
    new_id = torch.cumsum(used.long(), 0) - 1
    live = torch.zeros(B, dtype=torch.bool, device=dev)
    live[n_utt[used]] = True
    best = torch.where(live, best, torch.full_like(best, INF))
    piece = dict(n_v=n_v[used], n_q=n_q[used], alpha=alpha[used], beta=beta[used], src=new_id[src[kept]],
                 dst=new_id[dst[kept]], j=u['j'][kept], q=u['q'][kept], c=u['c'][kept])
    return piece, best, stats, redo


def _h64(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ----------------------------------------------------------------------------------
# shared: from kept pieces to the result's graph and arrays (torch ops, on either device)
# ----------------------------------------------------------------------------------
def _finish(pieces, dev, B, graph, blm, scale, time, state, arc, lp, node_utt):
    """pieces of disjoint utterances -> (RescoredGraph, the eight Lattice.FIELDS tensors, node and arc counts)"""
    Q = blm.num_states
    i64 = dict(dtype=torch.int64, device=dev)
    base, cat = 0, {k: [] for k in pieces[0]}
    for pc in pieces:
        for k, v in pc.items():
            v = torch.as_tensor(v).to(dev)
            cat[k].append(v + base if k in ('src', 'dst') else v)
        base += len(pc['n_v'])
    c = {k: torch.cat(v) for k, v in cat.items()}
    perm = torch.sort(c['n_v'] * Q + c['n_q'])[1]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(len(perm), **i64)
    n_v, n_q, alpha, beta = (c[k][perm] for k in ('n_v', 'n_q', 'alpha', 'beta'))
    src, dst = inv[c['src']], inv[c['dst']]
    order = torch.sort(src, stable=True)[1]
    src, dst, j, q, cost = (x[order] for x in (src, dst, c['j'], c['q'], c['c']))
    utt = node_utt[n_v]
    n_count = torch.bincount(utt, minlength=B)[:B] if len(utt) else torch.zeros(B, **i64)
    a_count = torch.bincount(utt[src], minlength=B)[:B] if len(src) else torch.zeros(B, **i64)
    n_off = torch.cumsum(n_count, 0) - n_count
    # the graph: distinct (state, q) pairs and distinct (graph arc, q) pairs
    skey = state.long()[n_v] * Q + n_q
    start_key = torch.tensor([graph.start * Q + blm.start()], **i64)
    pairs = torch.unique(torch.cat([skey, start_key]))
    new_state = torch.searchsorted(pairs, skey)
    a = arc.long()[j]
    akeys, a_inv = torch.unique(a * Q + q, return_inverse=True)
    m = int(akeys.numel())
    a_cost = torch.zeros(m, dtype=torch.float64, device=dev)
    a_cost[a_inv] = cost                                   # equal keys carry equal costs: any of them
    a_qd = torch.zeros(m, **i64)
    a_qd[a_inv] = n_q[dst]
    pairs_h, akeys_h, a_cost_h, a_qd_h = (x.cpu().numpy() for x in (pairs, akeys, a_cost, a_qd))
    ab, aq = akeys_h // Q, akeys_h % Q
    sid = np.searchsorted(pairs_h, graph.src[ab] * Q + aq)
    did = np.searchsorted(pairs_h, graph.dst[ab] * Q + a_qd_h)
    o = np.lexsort((ab, sid))
    rank = np.empty(m, np.int64)
    rank[o] = np.arange(m)
    rg = RescoredGraph(graph, blm, scale, np.stack([pairs_h // Q, pairs_h % Q], 1), sid[o], did[o], ab[o], aq[o],
                       a_cost_h[o])
    new_arc = torch.from_numpy(rank).to(dev)[a_inv] if m else a
    off_a = n_off[utt[src]] if len(src) else src
    fields = (time[n_v].int(), new_state.int(), alpha, beta, (src - off_a).int(), (dst - off_a).int(), new_arc,
              lp[j])
    return rg, fields, n_count.cpu().numpy(), a_count.cpu().numpy()


def _prepare(graph, lm, label_map, scale, oov_cost, max_lm_states):
    blm = BackoffLm.from_fst(lm)
    lmap = _default_label_map(graph, blm) if label_map is None else np.asarray(label_map, np.int64).reshape(-1)
    scale, oov_cost = float(scale), float(oov_cost)
    if not np.isfinite(scale) or np.isnan(oov_cost) or oov_cost == -INF:
        raise ValueError("rescore_lm: scale must be finite and oov_cost finite or +inf")
    cap = DEFAULT_MAX_LM_STATES if max_lm_states is None else int(max_lm_states)
    if not 1 <= cap <= DEVICE_MAX_LM_STATES:
        raise ValueError("max_lm_states must lie in [1, %d]" % DEVICE_MAX_LM_STATES)
    return blm, lmap, scale, oov_cost, cap


def _result_meta(B, n_count, best, reached):
    gone = n_count == 0
    return np.where(gone, np.float32(INF), best).astype(np.float32), np.where(gone, False, reached)


def rescore_lattices(lats, lm, label_map=None, scale=1.0, lattice_beam=None, oov_cost=INF, max_lm_states=None,
                     graph=None):
    """The numpy twin: a list of Lattice over one graph -> (list of Lattice over one RescoredGraph, stats)"""
    lats = list(lats)
    if graph is None:
        if not lats:
            raise ValueError("rescore_lm needs a lattice or the graph")
        graph = lats[0].graph
    blm, lmap, scale, oov_cost, _ = _prepare(graph, lm, label_map, scale, oov_cost, max_lm_states)
    view = _View(lats, graph)
    piece, best, st = _twin_piece(view, np.ones(view.B, bool), blm, lmap, scale, lattice_beam, oov_cost)
    t = torch.from_numpy
    rg, fields, n_count, a_count = _finish([piece], torch.device('cpu'), view.B, graph, blm, scale, t(view.time),
                                           t(view.state), t(view.arc), t(view.lp), t(view.node_utt))
    cost, reached = _result_meta(view.B, n_count, best, view.reached)
    out = _split(rg, fields, n_count, a_count, view.scale, view.frames, cost, reached)
    stats = dict(st, nodes_in=int(view.node_off[-1]), arcs_in=int(view.arc_off[-1]), nodes_out=int(n_count.sum()),
                 arcs_out=int(a_count.sum()), redone_on_host=[])
    return out, stats


def _split(rg, fields, n_count, a_count, scales, frames, cost, reached):
    host = [x.cpu().numpy() for x in fields]
    n_off, a_off = np.r_[0, np.cumsum(n_count)], np.r_[0, np.cumsum(a_count)]
    out = []
    for b in range(len(n_count)):
        ns, as_ = slice(n_off[b], n_off[b + 1]), slice(a_off[b], a_off[b + 1])
        out.append(Lattice(rg, scales[b], frames[b], cost[b], reached[b], *[x[ns] for x in host[:4]],
                           *[x[as_] for x in host[4:]]))
    return out


def rescore_device_batch(batch, lm, label_map=None, scale=1.0, lattice_beam=None, oov_cost=INF, max_lm_states=None,
                         workspace_bytes=None):
    """DeviceLatticeBatch.rescore_lm (att_speech.lattice_dp): see there"""
    from att_speech.lattice_dp import DeviceLatticeBatch
    graph, B, dev = batch.graph, batch.num_utterances, batch.device
    kw = dict(max_frames=batch.max_frames, num_classes=batch.num_classes, workspace_bytes=batch.workspace_bytes)
    if not batch._native_path('RESCORE') or B == 0 or batch.num_nodes == 0:
        lats, stats = rescore_lattices(batch.lattices(), lm, label_map, scale, lattice_beam, oov_cost, max_lm_states,
                                       graph=graph)
        blm = BackoffLm.from_fst(lm)
        rg = lats[0].graph if lats else RescoredGraph(graph, blm, scale, [[graph.start, blm.start()]], [], [], [], [], [])
        out = DeviceLatticeBatch.from_lattices(lats, dev, graph=rg, **kw)
        out.stats = stats
        return out
    blm, lmap, scale, oov_cost, cap = _prepare(graph, lm, label_map, scale, oov_cost, max_lm_states)
    L = _native.lib()
    if not L.asr_lattice_lmrescore_supported(batch.num_nodes, batch.num_arcs, batch.num_levels, cap):
        raise NotImplementedError("asr_lattice_lmrescore: the batch is too large")
    budget = int(batch.workspace_bytes if workspace_bytes is None else workspace_bytes)
    piece, best, st, redo = _device_piece(batch, blm, lmap, scale, lattice_beam, oov_cost, cap, budget)
    pieces = [piece]
    best = best.cpu().numpy()
    if redo:
        warnings.warn("rescore_lm: %d of %d utterances outgrew max_lm_states = %d LM states on a lattice node and "
                      "were redone on the host" % (len(redo), B, cap))
        view = _View(batch.lattices(), graph)
        select = np.zeros(B, bool)
        select[redo] = True
        hp, hbest, hst = _twin_piece(view, select, blm, lmap, scale, lattice_beam, oov_cost)
        pieces.append(hp)
        best = np.where(select, hbest, best)
        st = dict(max_lm_states=max(st['max_lm_states'], hst['max_lm_states']),
                  dropped_arcs=st['dropped_arcs'] + hst['dropped_arcs'])
    rg, fields, n_count, a_count = _finish(pieces, dev, B, graph, blm, scale, batch.time.long(), batch.state,
                                           batch.arc, batch.lp, batch.node_utt)
    cost, reached = _result_meta(B, n_count, best, batch.reached_final)
    out = DeviceLatticeBatch(rg, dev, *fields, n_count, a_count, batch.num_frames, reached, cost,
                             batch.acoustic_scale, **kw)
    out.stats = dict(st, nodes_in=batch.num_nodes, arcs_in=batch.num_arcs, nodes_out=int(n_count.sum()),
                     arcs_out=int(a_count.sum()), redone_on_host=redo)
    out.launches = batch.launches
    return out
