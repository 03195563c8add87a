"""Word lattices and n-best lists from the beam-pruned WFST search.

`decode_lattice` runs the search of att_speech.wfst_decode.decode_graph once and keeps, next to
the best path, every arc that lies within `lattice_beam` of it, with graph cost and acoustic score
apart on every arc: Kaldi's latgen-faster where the recipe ran decode-faster once per acoustic
scale (egs/wsj/ctc_kaldi_decode.sh:160-163).  A `Lattice` is re-ranked on the host
(`best_path(acoustic_scale=...)`: lattice-best-path) and listed (`nbest`: lattice-to-nbest), and
`sentences` has the shape AttentionDecoderTCN.score_sentences takes.

Semantics (order-independent, so the device kernel asr_wfst_lattice_f32,
the host path below and the tests' fp64 referee agree bit for bit).  The search is section 4.19's.
Time k = frames consumed; V_k the tokens after the closure at time k with costs alpha, S_k those
that survive the prune (S_n = V_n), thr_k the threshold of frame k's emitting phase.

  lattice arcs   emitting (k-1, s) -> (k, d): s in S_{k-1} and the proposal (alpha + w) + a_k[il]
                 is finite and <= thr_k; epsilon (k, s) -> (k, d): s, d in V_k, alpha + w finite
  beta           beta(n, s) = final(s) when a final state was reached, else 0 (allow_partial);
                 beta(u) = min over the lattice arcs u -> v of x + beta(v), x = w + a_k[il]
                 (w for epsilon arcs), fp32, one rounding per operation
  kept           alpha(u) + (x + beta(v)) <= best + lattice_beam (and finite), plus the arcs of
                 the search's own traceback
"""
import collections
import heapq
import os
import warnings

import numpy as np
import torch

from att_speech import _native
from att_speech.wfst_decode import DEFAULT_WORKSPACE_BYTES, _NOARC, _closure, _merge, _ranges

INF = float('inf')
DEFAULT_MAX_EXPANSIONS = 1 << 20

OVERFLOW_NAMES = {1: 'list', 2: 'log', 3: 'nodes', 4: 'arcs'}


class Lattice(object):
    """One utterance's pruned lattice in canonical form.

    Nodes sorted by (time, state): time, state [n_nodes] int32, alpha, beta [n_nodes] float32.
    Arcs sorted by (src node, graph arc index): src, dst (node indices), arc (the CSR position in
    `graph`) [n_arcs] int32/int64 and lp [n_arcs] float32, the raw class score the arc read (0 for
    epsilon arcs).  cost: the search's answer (+inf and no nodes: no lattice); reached_final: the
    end nodes are the final states of time num_frames (else every node of that time, cost 0)."""

    def __init__(self, graph, acoustic_scale, num_frames, cost, reached_final, time, state, alpha, beta,
                 src, dst, arc, lp):
        self.graph, self.acoustic_scale, self.num_frames = graph, float(acoustic_scale), int(num_frames)
        self.cost, self.reached_final = np.float32(cost), bool(reached_final)
        self.time, self.state = np.asarray(time, np.int32), np.asarray(state, np.int32)
        self.alpha, self.beta = np.asarray(alpha, np.float32), np.asarray(beta, np.float32)
        self.src, self.dst = np.asarray(src, np.int32), np.asarray(dst, np.int32)
        self.arc, self.lp = np.asarray(arc, np.int64), np.asarray(lp, np.float32)

    FIELDS = ('time', 'state', 'alpha', 'beta', 'src', 'dst', 'arc', 'lp')

    @property
    def num_nodes(self):
        return len(self.time)

    @property
    def num_arcs(self):
        return len(self.arc)

    @property
    def ilabel(self):
        return self.graph.ilabel[self.arc]

    @property
    def olabel(self):
        return self.graph.olabel[self.arc]

    @property
    def w(self):
        return self.graph.weight[self.arc]

    # ---- fp64 dynamic programmes over the DAG ---------------------------------------
    def _levels(self):
        """arc index groups by the (time, epsilon rank) of the source node, ascending"""
        R = self.graph.num_ranks + 1
        key = self.time[self.src].astype(np.int64) * R + self.graph.rank[self.state[self.src]]
        order = np.argsort(key, kind='stable')
        cuts = np.nonzero(np.r_[True, key[order][1:] != key[order][:-1]])[0] if len(order) else []
        return [order[a:b] for a, b in zip(cuts, list(cuts[1:]) + [len(order)])]

    def _arc_costs(self, acoustic_scale, lm_scale):
        sc = self.acoustic_scale if acoustic_scale is None else float(acoustic_scale)
        return float(lm_scale) * self.w.astype(np.float64) - sc * self.lp.astype(np.float64)

    def _end_costs(self, lm_scale):
        """per node: the cost of stopping there (+inf: not an end node)"""
        end = np.full(self.num_nodes, INF)
        at_n = self.time == self.num_frames
        if self.reached_final:
            end[at_n] = float(lm_scale) * self.graph.final[self.state[at_n]].astype(np.float64)
        else:
            end[at_n] = 0.0
        return end

    def best_path(self, acoustic_scale=None, lm_scale=1.0):
        """(words, cost, graph_cost, acoustic_cost) of the cheapest path when an arc costs
        lm_scale * w - acoustic_scale * lp and a final state lm_scale * final;
        cost = lm_scale * graph_cost + acoustic_scale * acoustic_cost.  acoustic_scale None: the
        scale of the search.  Equal costs: the smallest arc index into a node, then the smallest
        end state, as in the search.  No lattice: ([], inf, inf, inf)."""
        return LatticeBatch([self]).best_paths(acoustic_scale, lm_scale)[0]

    def posteriors(self, acoustic_scale=None, lm_scale=1.0):
        """LatticeBatch.posteriors of this lattice alone"""
        return LatticeBatch([self]).posteriors(acoustic_scale, lm_scale)

    def mbr(self, acoustic_scale=None, lm_scale=1.0, max_iterations=16, hypothesis=None, **kw):
        """LatticeBatch.mbr of this lattice alone: one MBRResult"""
        hyps = None if hypothesis is None else [hypothesis]
        return LatticeBatch([self]).mbr(acoustic_scale, lm_scale, max_iterations, hyps, **kw)[0]

    def nbest(self, n, acoustic_scale=None, lm_scale=1.0, max_expansions=DEFAULT_MAX_EXPANSIONS):
        """The n cheapest DISTINCT word sequences as [(words, cost)], sorted by (cost, words).

        Best-first over (node, word prefix) with the exact cost-to-go as the heuristic: all
        alignments of one word sequence meet in one search state, so each sequence comes out once,
        at its cheapest.  Sequences that tie at the n-th cost are all popped before the list is
        cut by (cost, words).  More than max_expansions pops raise RuntimeError."""
        n = int(n)
        if n < 1 or not self.num_nodes:
            return []
        x = self._arc_costs(acoustic_scale, lm_scale)
        end = self._end_costs(lm_scale)
        h = end.copy()
        for lv in reversed(self._levels()):
            cand = x[lv] + h[self.dst[lv]]
            ok = cand < INF
            np.minimum.at(h, self.src[lv][ok], cand[ok])
        start = np.nonzero((self.time == 0) & (self.state == self.graph.start))[0]
        if not len(start) or not h[start[0]] < INF:
            return []
        ptr = np.searchsorted(self.src, np.arange(self.num_nodes + 1))
        ol = self.olabel
        END = -1
        s0 = int(start[0])
        heap = [(float(h[s0]), (), s0, 0.0)]
        best_g = {(s0, ()): 0.0}
        done = set()
        out = []
        pops = 0
        while heap:
            f, words, v, gcost = heapq.heappop(heap)
            if (v, words) in done or gcost > best_g.get((v, words), INF):
                continue
            if len(out) >= n and f > out[-1][1]:
                break
            pops += 1
            if pops > max_expansions:
                raise RuntimeError("nbest: more than max_expansions = %d search states expanded for n = %d; "
                                   "raise max_expansions or lower n / lattice_beam" % (max_expansions, n))
            done.add((v, words))
            if v == END:
                out.append((list(words), gcost))
                continue
            if end[v] < INF:
                c = gcost + float(end[v])
                if c < best_g.get((END, words), INF):
                    best_g[(END, words)] = c
                    heapq.heappush(heap, (c, words, END, c))
            for j in range(int(ptr[v]), int(ptr[v + 1])):
                d = int(self.dst[j])
                if not h[d] < INF:
                    continue
                c = gcost + float(x[j])
                wd = words + (int(ol[j]),) if ol[j] != 0 else words
                if c < best_g.get((d, wd), INF):
                    best_g[(d, wd)] = c
                    heapq.heappush(heap, (c + float(h[d]), wd, d, c))
        out.sort(key=lambda e: (e[1], e[0]))
        return out[:n]

    def sentences(self, n, **kw):
        """the word lists of nbest(n), the shape AttentionDecoderTCN.score_sentences takes"""
        return [w for w, _ in self.nbest(n, **kw)]

    def oracle(self, reference, acoustic_scale=None, lm_scale=1.0):
        """LatticeBatch.oracle of this lattice alone: one OracleResult"""
        return LatticeBatch([self]).oracle([reference], acoustic_scale, lm_scale)[0]

    def depth(self):
        """emitting arcs per frame (Kaldi's lattice-depth); 0.0 for an empty lattice"""
        if not self.num_nodes or self.num_frames < 1:
            return 0.0
        return float(int((self.ilabel != 0).sum())) / float(self.num_frames)


NBEST_HASH_MUL = 0x9E3779B97F4A7C15     # H(o, h) = h * NBEST_HASH_MUL + o + 1 mod 2^64: LatticeBatch.nbest


# minimum-Bayes-risk decoding (LatticeBatch.mbr, asr_lattice_mbr_f64): the
# expected distances are int64 at 2^-40, the masses int64 at 2^-52, Kaldi's delta = 1e-5 is 10995116
MBR_ONE = 1 << 40
MBR_DELTA = 10995116
MBR_SUB = MBR_ONE + MBR_DELTA           # a substitution, and a lattice word matched to nothing
MBR_MASS = 1 << 52
MBR_TAU_SHIFT = 12

MBRResult = collections.namedtuple('MBRResult', 'words confidence frames risk iterations sausage')
MBRResult.__doc__ = """One utterance's minimum-Bayes-risk result: words, per word its confidence (the mass gamma
of its slot that agrees with it) and frame (the mass-weighted mean end time), risk (the expected word
edit distance of `words` under the lattice's path distribution; +inf: no lattice), iterations (the
number of evaluations) and sausage: per slot that holds a word or an alternative to a gap,
[(word, gamma)] sorted by (-gamma, word), word 0 standing for no word."""

MBR_NONE = MBRResult([], [], [], INF, 0, [])


def _mbr_frame(tau, gamma):
    """the frame of a word: tau = sum of (mass >> 12) * time over gamma's mass, to the nearest integer"""
    g = int(gamma) >> MBR_TAU_SHIFT
    return int(np.rint(float(int(tau)) / float(g))) if g > 0 else 0


def mbr_sausage(table):
    """the confusion network of {(slot, word): (gamma, tau)} (integers): per slot [(word, gamma)] by
    (-gamma, word); a gap slot whose only entry is word 0 is left out"""
    slots = {}
    for (q, w), (g, _) in table.items():
        if g > 0:
            slots.setdefault(q, []).append((int(w), float(int(g)) / MBR_MASS))
    sausage = []
    for q in sorted(slots):
        row = sorted(slots[q], key=lambda e: (-e[1], e[0]))
        if q % 2 == 1 and len(row) == 1 and row[0][0] == 0:
            continue
        sausage.append(row)
    return sausage


def mbr_result(words, risk, iterations, table):
    """an MBRResult from the words, the risk as int64 at 2^-40, and {(slot, word): (gamma, tau)} in
    integers"""
    conf, frames = [], []
    for k, w in enumerate(words):
        g, t = table.get((2 * k + 2, w), (0, 0))
        conf.append(float(int(g)) / MBR_MASS)
        frames.append(_mbr_frame(t, g))
    return MBRResult([int(w) for w in words], conf, frames, float(int(risk)) / MBR_ONE, int(iterations),
                     mbr_sausage(table))


# the lattice oracle (LatticeBatch.oracle, asr_lattice_oracle_i32): word edit distances
# are int32, ORACLE_UNREACHABLE stands for no path and every sum is clamped to it
ORACLE_UNREACHABLE = 1 << 30

OracleResult = collections.namedtuple('OracleResult', 'errors substitutions insertions deletions correct words '
                                                      'ref_frames cost')
OracleResult.__doc__ = """One utterance's lattice oracle: the least word edit distance `errors` between the reference
and any complete path of the lattice, split into substitutions, insertions (path words matched to nothing) and
deletions (reference words matched to nothing), with `correct` the matched words; `words` the word sequence of the
chosen path, ref_frames per reference word the end time of the arc it was aligned to (-1: deleted), and cost the
path's cost at the call's scales."""

ORACLE_NONE = OracleResult(-1, 0, 0, 0, 0, [], [], INF)

OracleErrorRate = collections.namedtuple('OracleErrorRate', 'errors reference_words rate skipped')


def oracle_error_rate(results, references):
    """(errors, reference_words, rate, skipped) over the utterances that have a result: the sums of their errors
    and reference lengths and the ratio of the two (0.0 over no reference words); the ORACLE_NONE utterances are
    left out of both sums and counted in `skipped`."""
    results, references = list(results), list(references)
    if len(results) != len(references):
        raise ValueError("oracle_error_rate: one reference per result")
    errors = words = skipped = 0
    for res, ref in zip(results, references):
        if res == ORACLE_NONE or res.errors < 0:
            skipped += 1
            continue
        errors += int(res.errors)
        words += len(ref)
    return OracleErrorRate(errors, words, float(errors) / words if words else 0.0, skipped)


def _oracle_references(references, B):
    if len(references) != B:
        raise ValueError("references must hold one word list per utterance")
    refs = [[int(w) for w in r] for r in references]
    if any(w <= 0 for r in refs for w in r):
        raise ValueError("references hold word labels > 0")
    return refs


def _oracle_arc_rows(Du, w, ref):
    """c_j(.) of in-arcs with source rows Du [k, R + 1] and words w [k] against the reference [R]"""
    U = ORACLE_UNREACHABLE
    step = np.minimum(Du + 1, U)
    c = step.copy()
    if Du.shape[1] > 1:
        c[:, 1:] = np.minimum(np.minimum(Du[:, :-1] + (w[:, None] != ref[None, :]), U), step[:, 1:])
    return np.where((w != 0)[:, None], c, Du)


def _oracle_path(lat, ref):
    """the oracle path of one Lattice against the labels `ref`: None, or (errors, (substitutions, insertions,
    deletions, correct), ref_frames, the path's lattice arcs in forward order, its end node); the semantics
    include/asr_amd.h states for asr_lattice_oracle_i32"""
    U = ORACLE_UNREACHABLE
    n, R, g = lat.num_nodes, len(ref), lat.graph
    if not n:
        return None
    start = np.nonzero((lat.time == 0) & (lat.state == g.start))[0]
    if not len(start):
        return None
    s = int(start[0])
    level = lat.time.astype(np.int64) * (g.num_ranks + 1) + g.rank[lat.state]
    order = np.argsort(level, kind='stable')
    cuts = np.nonzero(np.r_[True, level[order][1:] != level[order][:-1]])[0]
    if len(cuts) + R >= U:
        raise ValueError("oracle: the levels of the lattice plus the reference must stay below 2^30")
    src, dst, ol = lat.src.astype(np.int64), lat.dst.astype(np.int64), lat.olabel.astype(np.int64)
    in_arc = np.argsort(dst, kind='stable')             # a node's in-arcs in arc order
    in_ptr = np.searchsorted(dst[in_arc], np.arange(n + 1))
    ref = np.asarray(ref, np.int64)
    col = np.arange(R + 1, dtype=np.int64)
    D = np.full((n, R + 1), U, np.int64)
    D[s] = col
    for a, b in zip(cuts, list(cuts[1:]) + [n]):
        V = order[a:b]
        V = V[(V != s) & (in_ptr[V + 1] > in_ptr[V])]
        if not len(V):
            continue
        pos, owner = _ranges(in_ptr[V], in_ptr[V + 1])
        arcs = in_arc[pos]
        c = _oracle_arc_rows(D[src[arcs]], ol[arcs], ref)
        first = np.nonzero(np.r_[True, owner[1:] != owner[:-1]])[0]
        D0 = np.minimum.reduceat(c, first, axis=0)
        D[V] = np.minimum(col + np.minimum.accumulate(D0 - col, axis=1), U)
    at_n = lat.time == lat.num_frames
    is_end = at_n & (g.final[lat.state] < INF) if lat.reached_final else at_n
    ends = np.nonzero(is_end)[0]
    if not len(ends) or int(D[ends, R].min()) >= U:
        return None
    errors = int(D[ends, R].min())
    v = last = int(ends[np.nonzero(D[ends, R] == errors)[0][0]])
    q = R
    n_sub = n_ins = n_del = n_cor = 0
    frames = [0] * R
    path = []
    while v != s:
        js = in_arc[in_ptr[v]:in_ptr[v + 1]]
        hit = np.nonzero(_oracle_arc_rows(D[src[js]], ol[js], ref)[:, q] == D[v, q])[0] if len(js) else []
        if not len(hit):
            frames[q - 1] = -1
            n_del += 1
            q -= 1
            continue
        j = int(js[hit[0]])
        u, w = int(src[j]), int(ol[j])
        path.append(j)
        if w != 0 and q >= 1 and min(int(D[u, q - 1]) + (w != ref[q - 1]), U) == D[v, q]:
            if w == ref[q - 1]:
                n_cor += 1
            else:
                n_sub += 1
            frames[q - 1] = int(lat.time[v])
            q -= 1
        elif w != 0:
            n_ins += 1
        v = u
    for k in range(q):
        frames[k] = -1
    n_del += q
    path.reverse()
    return errors, (n_sub, n_ins, n_del, n_cor), frames, path, last


def _oracle_one(lat, ref, acoustic_scale, lm_scale):
    found = _oracle_path(lat, ref)
    if found is None:
        return ORACLE_NONE
    errors, (n_sub, n_ins, n_del, n_cor), frames, path, last = found
    g, ol = lat.graph, lat.olabel
    sc = lat.acoustic_scale if acoustic_scale is None else float(acoustic_scale)
    lm = float(lm_scale)
    with np.errstate(invalid='ignore', over='ignore'):
        x = lm * lat.w.astype(np.float64) - sc * lat.lp.astype(np.float64)
        total = np.float64(0.0)
        for j in path:
            total = total + x[j]
        end = np.float64(lm) * np.float64(g.final[lat.state[last]]) if lat.reached_final else np.float64(0.0)
        cost = float(total + end)
    return OracleResult(errors, n_sub, n_ins, n_del, n_cor, [int(ol[j]) for j in path if ol[j] != 0], frames, cost)


class _Entries(object):
    """the n-best entries of all nodes, one after another, in arrays that grow"""

    NAMES = (('c', np.float64), ('ln', np.int64), ('h', np.uint64), ('arc', np.int64), ('rank', np.int64))

    def __init__(self):
        self.used = 0
        for name, dtype in self.NAMES:
            setattr(self, name, np.zeros(1024, dtype))

    def append(self, *columns):
        k = len(columns[0])
        for (name, dtype), col in zip(self.NAMES, columns):
            a = getattr(self, name)
            if self.used + k > len(a):
                a = np.concatenate([a, np.zeros(max(len(a), k), dtype)])
                setattr(self, name, a)
            a[self.used:self.used + k] = col
        self.used += k


def nbest_lists(num_utterances, utt, words, cost):
    """entries (utterance, words, cost) -> per utterance [(words, cost)] sorted by (cost, words)"""
    out = [[] for _ in range(num_utterances)]
    for b, w, c in zip(utt, words, cost):
        out[b].append((w, c))
    for row in out:
        row.sort(key=lambda entry: (entry[1], entry[0]))
    return out


class LatticeBatch(object):
    """The lattices of many utterances over one graph, laid end to end, so that one dynamic
    programme serves them all: a sweep over acoustic scales builds this once and calls best_paths
    once per scale."""

    def __init__(self, lattices):
        self.lattices = lats = list(lattices)
        if not lats:
            return
        g = self.graph = lats[0].graph
        nn = np.array([l.num_nodes for l in lats], np.int64)
        na = np.array([l.num_arcs for l in lats], np.int64)
        self.node_off = np.r_[0, np.cumsum(nn)]
        self.n_utt = np.repeat(np.arange(len(lats)), nn)
        a_utt = np.repeat(np.arange(len(lats)), na)
        cat = np.concatenate
        self.time, self.state = cat([l.time for l in lats]).astype(np.int64), cat([l.state for l in lats])
        self.src = cat([l.src for l in lats]).astype(np.int64) + self.node_off[a_utt]
        self.dst = cat([l.dst for l in lats]).astype(np.int64) + self.node_off[a_utt]
        self.arc, self.lp = cat([l.arc for l in lats]), cat([l.lp for l in lats]).astype(np.float64)
        self.w = g.weight[self.arc].astype(np.float64)
        self.ol = g.olabel[self.arc]
        self.scale = cat([np.full(k, l.acoustic_scale) for k, l in zip(na, lats)]) if len(lats) else None
        self.start = (self.time == 0) & (self.state == g.start)
        frames = np.array([l.num_frames for l in lats], np.int64)
        reached = np.array([l.reached_final for l in lats], bool)
        at_n = self.time == frames[self.n_utt]
        # the unscaled cost of stopping at a node (+inf: not an end node)
        self.end = np.where(at_n, np.where(reached[self.n_utt], g.final[self.state].astype(np.float64), 0.0), INF)
        self.free_end = at_n & ~reached[self.n_utt]      # end nodes of a partial lattice: 0 whatever the LM scale
        # arcs grouped by the (time, epsilon rank) of their source, ascending: a node's cost is final
        # before its arcs are relaxed
        key = self.time[self.src] * (g.num_ranks + 1) + g.rank[self.state[self.src]]
        order = np.argsort(key, kind='stable')
        cuts = np.nonzero(np.r_[True, key[order][1:] != key[order][:-1]])[0] if len(order) else []
        # within a level the arcs are grouped by destination, so a level is one minimum.reduceat
        self.levels = []
        for a, b in zip(cuts, list(cuts[1:]) + [len(order)]):
            lv = order[a:b]
            lv = lv[np.argsort(self.dst[lv], kind='stable')]
            d = self.dst[lv]
            first = np.nonzero(np.r_[True, d[1:] != d[:-1]])[0]
            self.levels.append((lv, self.src[lv], first, d[first]))

    def best_paths(self, acoustic_scale=None, lm_scale=1.0):
        """Lattice.best_path for every lattice: a list of (words, cost, graph_cost, acoustic_cost)"""
        return self._best_paths(acoustic_scale, lm_scale)[0]

    def rescore_lm(self, lm, label_map=None, scale=1.0, lattice_beam=None, oov_cost=INF, max_lm_states=None,
                   workspace_bytes=None, graph=None):
        """lattice o back-off n-gram LM: a LatticeBatch over a RescoredGraph, with `stats`.  The numpy twin
        of DeviceLatticeBatch.rescore_lm, bit for bit (att_speech.lattice_lm states the semantics;
        max_lm_states and workspace_bytes only bound the device path)."""
        from att_speech.lattice_lm import rescore_lattices
        lats, stats = rescore_lattices(self.lattices, lm, label_map, scale, lattice_beam, oov_cost, max_lm_states,
                                       graph=graph)
        out = LatticeBatch(lats)
        out.stats = stats
        return out

    def _best_paths(self, acoustic_scale=None, lm_scale=1.0):
        """(best_paths' list, per utterance the batch arc indices of the path's word-bearing arcs)"""
        none = ([], INF, INF, INF)
        if not self.lattices:
            return [], []
        B, N = len(self.lattices), len(self.time)
        if not N:
            return [none] * B, [[] for _ in range(B)]
        sc = self.scale if acoustic_scale is None else float(acoustic_scale)
        x = float(lm_scale) * self.w - sc * self.lp
        cost = np.where(self.start, 0.0, INF)
        for lv, src, first, dst in self.levels:
            cost[dst] = np.minimum(cost[dst], np.minimum.reduceat(cost[src] + x[lv], first))
        cand = cost[self.src] + x
        win = np.nonzero((cand == cost[self.dst]) & (cand < INF))[0]
        # of the arcs that attain a node's cost, the smallest GRAPH arc index (not lattice position)
        garc = np.full(N, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(garc, self.dst[win], self.arc[win])
        hit = win[self.arc[win] == garc[self.dst[win]]]
        bp = np.full(N, -1, np.int64)
        bp[self.dst[hit]] = hit
        bp[self.start] = -1
        tot = cost + float(lm_scale) * self.end
        best = np.full(B, INF)
        np.minimum.at(best, self.n_utt, tot)
        # the first node that attains it: nodes are sorted by state within a time
        v = np.full(B, N, np.int64)
        at = np.nonzero((tot == best[self.n_utt]) & (tot < INF))[0]
        np.minimum.at(v, self.n_utt[at], at)
        live = v < N
        gc = np.zeros(B)
        gc[live] = np.where(self.end[v[live]] < INF, self.end[v[live]], 0.0)
        ac = np.zeros(B)
        cur = np.where(live, v, 0)
        w_utt, w_lab, w_step, w_arc = [], [], [], []
        for step in range(len(self.levels) + 1):       # a path has at most one arc per level
            j = np.where(live, bp[cur], -1)
            live = j >= 0
            if not live.any():
                break
            u = np.nonzero(live)[0]
            ju = j[u]
            gc[u] += self.w[ju]
            ac[u] -= self.lp[ju]
            has = self.ol[ju] != 0
            w_utt.append(u[has])
            w_lab.append(self.ol[ju][has])
            w_arc.append(ju[has])
            w_step.append(np.full(int(has.sum()), step))
            cur[u] = self.src[ju]
        words = [[] for _ in range(B)]
        arcs = [[] for _ in range(B)]
        if w_utt:
            wu, wl, ws = np.concatenate(w_utt), np.concatenate(w_lab), np.concatenate(w_step)
            wa = np.concatenate(w_arc)
            for i in np.lexsort((-ws, wu)):             # per utterance, the last step first: path order
                words[wu[i]].append(int(wl[i]))
                arcs[wu[i]].append(int(wa[i]))
        return ([(words[b], float(best[b]), float(gc[b]), float(ac[b])) if best[b] < INF else none
                 for b in range(B)], [arcs[b] if best[b] < INF else [] for b in range(B)])

    def nbest(self, n, acoustic_scale=None, lm_scale=1.0):
        """The n cheapest DISTINCT word sequences of every lattice: one [(words, cost)] per utterance,
        sorted by (cost, words).  The k-best dynamic programme of DESIGN.md section 4.22, and the
        numpy twin of asr_lattice_nbest_f64, operation for operation, so both give the same bits.

        Backwards over the (time, epsilon rank) levels every node v keeps a list of at most n
        entries (c, len, h, arc, rank): the cost of a word suffix from v to an end, its number of
        words, a 64-bit hash of it, the out-arc taken (-1: stop at v) and the index into the list
        of that arc's destination.  Candidates of v: the stop entry (e(v), 0, 0, -1, 0) when
        e(v) < inf (e as in Lattice._end_costs), and for every out-arc j and entry r of its
        destination (fl(x_j + c_r), len_r + [olabel_j != 0], H(olabel_j, h_r), j, r), dropped unless
        the cost is < inf (NaN goes too); x_j = fl(fl(lm w) - fl(sc lp)) as in best_paths.
        H(o, h) = h * 0x9E3779B97F4A7C15 + o + 1 mod 2^64 for o != 0, h otherwise; the empty suffix
        hashes to 0.  The candidates are ordered by (c, len, h, arc, rank); of those with equal
        (len, h) the first survives; the list is the first n survivors.

        Read-out: the start node's entries are followed forwards along (arc, rank), the non-zero
        output labels collected, and the cost summed forwards (g = 0; g = fl(g + x_j); fl(g + e)) as
        Lattice.nbest and best_paths sum it.

        Two suffixes count as the same sequence iff (len, h) agree: a 64-bit hash identity.  A
        collision would drop one of two different sequences from a list and nothing else.  Against
        Lattice.nbest: the same costs; sequences that tie at the n-th cost are cut by (len, hash)
        here and by the words there."""
        B = len(self.lattices)
        n = int(n)
        N = len(self.time) if B else 0
        if n < 1 or not N:
            return [[] for _ in range(B)]
        g = self.graph
        sc = self.scale if acoustic_scale is None else float(acoustic_scale)
        lm = float(lm_scale)
        mul, one = np.uint64(NBEST_HASH_MUL), np.uint64(1)
        with np.errstate(invalid='ignore', over='ignore'):
            x = lm * self.w - sc * self.lp
            e = np.where(self.end < INF, np.where(self.free_end, 0.0, lm * np.where(self.end < INF, self.end, 0.0)),
                         INF)
            level = self.time * (g.num_ranks + 1) + g.rank[self.state]
            order = np.argsort(-level, kind='stable')
            cuts = np.nonzero(np.r_[True, level[order][1:] != level[order][:-1]])[0]
            out_ptr = np.searchsorted(self.src, np.arange(N + 1))
            off, cnt = np.zeros(N, np.int64), np.zeros(N, np.int64)
            ent = _Entries()
            for a, b in zip(cuts, list(cuts[1:]) + [N]):
                V = order[a:b]
                arcs, owner = _ranges(out_ptr[V], out_ptr[V + 1])
                d = self.dst[arcs]
                pos, which = _ranges(off[d], off[d] + cnt[d])
                ca, ol = arcs[which], self.ol[arcs[which]]
                word = ol != 0
                c = x[ca] + ent.c[pos]
                h = np.where(word, ent.h[pos] * mul + ol.astype(np.int64).astype(np.uint64) + one, ent.h[pos])
                ok = c < INF
                stop = V[e[V] < INF]
                zero = np.zeros(len(stop), np.int64)
                node = np.r_[V[owner[which]][ok], stop]
                c = np.r_[c[ok], e[stop]]
                ln = np.r_[(ent.ln[pos] + word)[ok], zero]
                h = np.r_[h[ok], zero.astype(np.uint64)]
                arc = np.r_[ca[ok], zero - 1]
                rank = np.r_[(pos - off[d][which])[ok], zero]
                o = np.lexsort((rank, arc, h, ln, c, node))
                node, c, ln, h, arc, rank = (v[o] for v in (node, c, ln, h, arc, rank))
                # of equal (node, len, h) the first in that order; lexsort is stable
                o = np.lexsort((h, ln, node))
                same = (node[o][1:] == node[o][:-1]) & (ln[o][1:] == ln[o][:-1]) & (h[o][1:] == h[o][:-1])
                keep = np.zeros(len(o), bool)
                keep[o[np.r_[True, ~same][:len(o)]]] = True
                node, c, ln, h, arc, rank = (v[keep] for v in (node, c, ln, h, arc, rank))
                first = np.nonzero(np.r_[True, node[1:] != node[:-1]][:len(node)])[0]
                run = np.diff(np.r_[first, len(node)])
                keep = np.arange(len(node)) - np.repeat(first, run) < n
                u, at, k = np.unique(node[keep], return_index=True, return_counts=True)
                off[u], cnt[u] = ent.used + at, k
                ent.append(c[keep], ln[keep], h[keep], arc[keep], rank[keep])
            # read-out: every entry of every start node, all chains at once
            start = np.full(B, N, np.int64)
            at = np.nonzero(self.start)[0]
            np.minimum.at(start, self.n_utt[at], at)
            utts = np.nonzero(start < N)[0]
            pos, which = _ranges(off[start[utts]], off[start[utts]] + cnt[start[utts]])
            utt = utts[which]
            node = start[utt]
            total, cost = np.zeros(len(pos)), np.full(len(pos), INF)
            live = np.ones(len(pos), bool)
            w_ent, w_lab = [], []
            for _ in range(len(cuts) + 1):              # a path has at most one arc per level
                arc = ent.arc[pos]
                ends = live & (arc < 0)
                cost[ends] = total[ends] + e[node[ends]]
                live = live & (arc >= 0)
                i = np.nonzero(live)[0]
                if not len(i):
                    break
                j = arc[i]
                total[i] = total[i] + x[j]
                has = self.ol[j] != 0
                w_ent.append(i[has])
                w_lab.append(self.ol[j][has])
                pos[i] = off[self.dst[j]] + ent.rank[pos[i]]
                node[i] = self.dst[j]
        words = [[] for _ in range(len(pos))]
        if w_ent:                                       # step by step: every entry's words in path order
            for i, lab in zip(np.concatenate(w_ent).tolist(), np.concatenate(w_lab).tolist()):
                words[i].append(int(lab))
        return nbest_lists(B, utt.tolist(), words, cost.tolist())

    def posteriors(self, acoustic_scale=None, lm_scale=1.0):
        """Arc and node posteriors of every lattice under the path weights exp(-(sum of x + lm_scale *
        end)), x = lm_scale * w - acoustic_scale * lp as in best_paths: one log-semiring
        forward-backward in fp64 over the levels.  Returns a LatticePosteriors.  A final cost of +inf
        ends no path, whatever lm_scale is."""
        B = len(self.lattices)
        N = len(self.time) if B else 0
        if not N:
            return LatticePosteriors(self, np.full(B, -INF), np.zeros(0), np.zeros(0), acoustic_scale, lm_scale)
        sc = self.scale if acoustic_scale is None else float(acoustic_scale)
        lm = float(lm_scale)
        x = lm * self.w - sc * self.lp
        fwd = np.where(self.start, 0.0, -INF)
        with np.errstate(invalid='ignore'):
            stop = np.where(self.end < INF, -(lm * np.where(self.end < INF, self.end, 0.0)), -INF)
            bwd = stop.copy()
            for lv, src, _, _ in self.levels:
                ok = fwd[src] > -INF
                np.logaddexp.at(fwd, self.dst[lv][ok], fwd[src][ok] - x[lv][ok])
            for lv, src, _, _ in reversed(self.levels):
                d = self.dst[lv]
                ok = bwd[d] > -INF
                np.logaddexp.at(bwd, src[ok], bwd[d][ok] - x[lv][ok])
            first = np.full(B, N, np.int64)
            np.minimum.at(first, self.n_utt[self.start], np.nonzero(self.start)[0])
            log_z = np.where(first < N, bwd[np.minimum(first, N - 1)], -INF)
            zn = log_z[self.n_utt]
            node = np.where((fwd > -INF) & (bwd > -INF) & (zn > -INF), fwd + bwd - zn, -INF)
            a_utt = self.n_utt[self.src]
            za = log_z[a_utt]
            part = fwd[self.src] - x
            arc = np.where((fwd[self.src] > -INF) & (bwd[self.dst] > -INF) & (za > -INF),
                           part + bwd[self.dst] - za, -INF)
        return LatticePosteriors(self, log_z, arc, node, acoustic_scale, lm_scale)

    # ---- sequence-discriminative training statistics -----------------------------------------------
    def seq_objective(self, log_probs, ref=None, criterion='mmi', acoustic_scale=None, lm_scale=1.0, boost=0.0):
        """The lattice MMI / boosted MMI denominator or the sMBR objective of every lattice, from the LIVE
        scores: the numpy twin of asr_lattice_seqtrain_f64 (include/asr_amd.h states the semantics; DESIGN.md
        section 4.26), fp64, level by level.

        log_probs [T, B, C] float32 or float64 (array or tensor); ref [B, T] integer classes per frame
        (CTCAlignment.frames; -1 never matches) or None (every accuracy 0).  An emitting arc into time k
        scores s = log_probs[k - 1, b, ilabel - 1] (the stored lp is not read), acc = (ref[b, k - 1] ==
        ilabel - 1), and costs x = lm_scale w - acoustic_scale s + boost acc.

        Returns (objective [B] f64, arc_grad [arcs] f64, occ [T, B, C] float32):
          'mmi'   log_z and the arc posteriors gamma;
          'smbr'  the expected frame accuracy c_avg and gamma (c(a) - c_avg);
        occ: arc_grad summed in fp64 per (frame, class) in ascending arc order, rounded once;
        d objective[b] / d log_probs[t, b, c] = acoustic_scale occ[t, b, c].  An utterance without a
        complete path has objective -inf ('mmi') or 0 ('smbr') and zero arc_grad and occ."""
        if criterion not in ('mmi', 'smbr'):
            raise ValueError("criterion must be 'mmi' or 'smbr', not %r" % (criterion,))
        if not float(boost) >= 0.0 or float(boost) == INF:
            raise ValueError("boost must be finite and >= 0")
        lpr = log_probs.detach().cpu().numpy() if isinstance(log_probs, torch.Tensor) else np.asarray(log_probs)
        if lpr.ndim != 3:
            raise ValueError("log_probs must be [T, B, C]")
        T, B, C = lpr.shape
        if B != len(self.lattices):
            raise ValueError("log_probs has %d utterances, the batch %d" % (B, len(self.lattices)))
        smbr = criterion == 'smbr'
        objective = np.full(B, 0.0 if smbr else -INF)
        occ = np.zeros((T, B, C), np.float32)
        A = len(self.arc) if B else 0
        if ref is not None:
            ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
            if ref.shape != (B, T):
                raise ValueError("ref must be [B, T] = %s, not %s" % ((B, T), tuple(ref.shape)))
        if not B or not len(self.time):
            return objective, np.zeros(A), occ
        N = len(self.time)
        il = self.graph.ilabel[self.arc].astype(np.int64)
        k = self.time[self.dst]
        a_utt = self.n_utt[self.src]
        em = il > 0
        if ((il[em] > C) | (k[em] > T) | (k[em] < 1)).any():
            raise ValueError("seq_objective: the lattice has classes or frames beyond [T, B, C] = %s" % ((T, B, C),))
        s = np.zeros(A)
        acc = np.zeros(A)
        s[em] = lpr[k[em] - 1, a_utt[em], il[em] - 1].astype(np.float64)
        if ref is not None:
            acc[em] = (ref[a_utt[em], k[em] - 1] == il[em] - 1).astype(np.float64)
        sc = self.scale if acoustic_scale is None else float(acoustic_scale)
        lm = float(lm_scale)
        with np.errstate(invalid='ignore', over='ignore'):
            x = lm * self.w - sc * s + float(boost) * acc
            fwd = np.where(self.start, 0.0, -INF)
            stop = np.where(self.end < INF, -(lm * np.where(self.end < INF, self.end, 0.0)), -INF)
            bwd = stop.copy()
            for lv, src, _, _ in self.levels:
                ok = (fwd[src] > -INF) & (x[lv] < INF)
                np.logaddexp.at(fwd, self.dst[lv][ok], fwd[src][ok] - x[lv][ok])
            for lv, src, _, _ in reversed(self.levels):
                d = self.dst[lv]
                ok = (bwd[d] > -INF) & (x[lv] < INF)
                np.logaddexp.at(bwd, src[ok], bwd[d][ok] - x[lv][ok])
            # expected accuracies: a node's value is complete before its own arcs are taken
            facc, bacc = np.zeros(N), np.zeros(N)
            for lv, src, _, _ in self.levels:
                d = self.dst[lv]
                ok = (fwd[src] > -INF) & (x[lv] < INF) & (fwd[d] > -INF)
                lv, src, d = lv[ok], src[ok], d[ok]
                np.add.at(facc, d, np.exp(fwd[src] - x[lv] - fwd[d]) * (facc[src] + acc[lv]))
            for lv, src, _, _ in reversed(self.levels):
                d = self.dst[lv]
                ok = (bwd[d] > -INF) & (x[lv] < INF) & (bwd[src] > -INF)
                lv, src, d = lv[ok], src[ok], d[ok]
                np.add.at(bacc, src, np.exp(bwd[d] - x[lv] - bwd[src]) * (bacc[d] + acc[lv]))
            first = np.full(B, N, np.int64)
            np.minimum.at(first, self.n_utt[self.start], np.nonzero(self.start)[0])
            at = np.minimum(first, N - 1)
            log_z = np.where(first < N, bwd[at], -INF)
            have = log_z > -INF
            c_avg = np.where(have, bacc[at], 0.0)
            za = log_z[a_utt]
            live = (fwd[self.src] > -INF) & (x < INF) & (bwd[self.dst] > -INF) & (za > -INF)
            gamma = np.where(live, np.exp(np.where(live, fwd[self.src] - x + bwd[self.dst] - za, 0.0)), 0.0)
        if smbr:
            objective = c_avg
            arc_grad = np.where(live, gamma * ((facc[self.src] + acc + bacc[self.dst]) - c_avg[a_utt]), 0.0)
        else:
            objective = log_z
            arc_grad = gamma
        flat = ((k[em] - 1) * B + a_utt[em]) * C + (il[em] - 1)
        sums = np.zeros(T * B * C)
        np.add.at(sums, flat, arc_grad[em])     # unbuffered: the arcs of an entry in ascending order
        return objective, arc_grad, sums.reshape(T, B, C).astype(np.float32)

    # ---- the lattice oracle ---------------------------------------------------------------------
    def oracle(self, references, acoustic_scale=None, lm_scale=1.0):
        """The lattice oracle (Kaldi's lattice-oracle): per utterance the complete path whose words are
        nearest to the reference (a list of labels > 0) in word edit distance, as an OracleResult; ORACLE_NONE
        where the lattice has no complete path.  The numpy twin of asr_lattice_oracle_i32 (include/asr_amd.h
        states the semantics), in the same integer arithmetic, so both give the same
        results with ==.

        D(v, q), the least distance between the words of a path from the start node to v and the first q
        reference labels, is computed level by level: per in-arc (u -> v, w) in arc order c(q) = D(u, q) for
        w = 0, else min(D(u, q - 1) + [w != r_q], D(u, q) + 1); D0 = min over the in-arcs; D(v, q) =
        min(D0(v, q), D(v, q - 1) + 1).  errors = min over the end nodes of D(v, R), the smallest node among
        the minima; the traceback takes the first in-arc that attains D(v, q), a diagonal step before an
        insertion, and a deletion only when no in-arc attains it.  Ties among paths of the least distance are
        broken by that rule, not by cost; cost is summed forwards as nbest sums it."""
        refs = _oracle_references(references, len(self.lattices))
        return [_oracle_one(lat, ref, acoustic_scale, lm_scale) for lat, ref in zip(self.lattices, refs)]

    def depth(self):
        """per utterance the emitting arcs per frame (Kaldi's lattice-depth); 0.0 for an empty lattice"""
        return [lat.depth() for lat in self.lattices]

    # ---- minimum-Bayes-risk decoding ---------------------------------------------------------
    def conditionals(self, acoustic_scale=None, lm_scale=1.0):
        """(arc_cond [arcs], end_cond [nodes]) in linear fp64: the probability of in-arc j given that a
        path passes through its destination, exp((fwd(src) - x) - fwd(dst)), and of stopping at node v
        given a complete path, exp((fwd(v) - fl(lm end(v))) - log_z); fwd as in posteriors.  0 where
        a term is infinite."""
        B = len(self.lattices)
        N = len(self.time) if B else 0
        if not N:
            return np.zeros(0), np.zeros(0)
        sc = self.scale if acoustic_scale is None else float(acoustic_scale)
        lm = float(lm_scale)
        x = lm * self.w - sc * self.lp
        fwd = np.where(self.start, 0.0, -INF)
        with np.errstate(invalid='ignore', over='ignore'):
            for lv, src, _, _ in self.levels:
                ok = fwd[src] > -INF
                np.logaddexp.at(fwd, self.dst[lv][ok], fwd[src][ok] - x[lv][ok])
            is_end = (self.end < INF) & (fwd > -INF)
            stop = np.where(is_end, fwd - lm * np.where(self.end < INF, self.end, 0.0), -INF)
            log_z = np.full(B, -INF)
            np.logaddexp.at(log_z, self.n_utt[is_end], stop[is_end])
            end_cond = np.where(stop > -INF, np.exp(stop - log_z[self.n_utt]), 0.0)
            ok = (fwd[self.src] > -INF) & (x < INF) & (fwd[self.dst] > -INF)
            arc_cond = np.where(ok, np.exp((fwd[self.src] - x) - fwd[self.dst]), 0.0)
        return np.where(arc_cond > 0, arc_cond, 0.0), np.where(end_cond > 0, end_cond, 0.0)

    def mbr(self, acoustic_scale=None, lm_scale=1.0, max_iterations=16, hypotheses=None, arc_cond=None,
            end_cond=None):
        """Minimum-Bayes-risk decoding (Xu, Povey, Mangu, Zhu 2011; Kaldi's lattice-mbr-decode): per
        utterance the word sequence that minimises the expected word edit distance under the lattice's
        path distribution at these scales, with per-word confidences, frames and the confusion network.
        One MBRResult per utterance.  The numpy twin of asr_lattice_mbr_f64 (include/asr_amd.h states
        the semantics), in the same integer arithmetic, so both give the same results with ==.

        Start: `hypotheses` (a word list per utterance) or the best path's words.  Every evaluation is
        an edit-distance forward-backward over (node, hypothesis slot); then every slot takes the
        word of the largest mass gamma (ties: the current word, else the smallest label).  It stops
        when the words did not change or after max(1, max_iterations) evaluations; the result is the
        last evaluated hypothesis's, so max_iterations=0 with hypotheses scores them unchanged.
        arc_cond / end_cond override conditionals().  No lattice or no complete path: MBR_NONE."""
        B = len(self.lattices)
        N = len(self.time) if B else 0
        if hypotheses is not None and len(hypotheses) != B:
            raise ValueError("hypotheses must hold one word list per utterance")
        if not N:
            return [MBR_NONE] * B
        if arc_cond is None or end_cond is None:
            ac, ec = self.conditionals(acoustic_scale, lm_scale)
            arc_cond = ac if arc_cond is None else arc_cond
            end_cond = ec if end_cond is None else end_cond
        pi, pe = np.asarray(arc_cond, np.float64), np.asarray(end_cond, np.float64)
        if len(pi) != len(self.arc) or len(pe) != N:
            raise ValueError("arc_cond / end_cond must have one entry per arc / node")
        pi, pe = np.where(pi > 0, pi, 0.0), np.where(pe > 0, pe, 0.0)
        first = np.full(B, N, np.int64)
        np.minimum.at(first, self.n_utt[self.start], np.nonzero(self.start)[0])
        live = first < N
        ends = np.zeros(B, bool)
        ends[self.n_utt[pe > 0]] = True
        live &= ends
        if hypotheses is None:
            with np.errstate(invalid='ignore'):
                best = self.best_paths(acoustic_scale, lm_scale)
            hyps = [list(w) for w, _, _, _ in best]
            live &= np.array([c < INF for _, c, _, _ in best])
        else:
            hyps = [[int(w) for w in h] for h in hypotheses]
            if any(w <= 0 for h in hyps for w in h):
                raise ValueError("hypotheses hold word labels > 0")
        n_max = max(1, int(max_iterations))
        results = [MBR_NONE] * B
        iters = np.zeros(B, np.int64)
        while live.any():
            risk, tables = self._mbr_evaluate(hyps, live, pi, pe, first)
            for b in np.nonzero(live)[0].tolist():
                iters[b] += 1
                new = hyps[b]
                if iters[b] < n_max:
                    new = mbr_update(hyps[b], tables[b])
                if new == hyps[b]:
                    results[b] = mbr_result(hyps[b], risk[b], iters[b], tables[b])
                    live[b] = False
                hyps[b] = new
        return results

    def _mbr_evaluate(self, hyps, live, pi, pe, first):
        """one edit-distance forward-backward of the live utterances: (risk [B] int64 at 2^-40, per
        utterance {(slot, word): (gamma, tau)})"""
        B, N = len(self.lattices), len(self.time)
        i64 = np.int64
        S = np.array([2 * len(h) + 1 if live[b] else 0 for b, h in enumerate(hyps)], i64)
        C = int(S.max()) + 1
        col = np.arange(C)
        R = np.zeros((B, C), i64)
        for b in np.nonzero(live)[0]:
            R[b, 2:S[b]:2] = hyps[b]
        dl = np.where(R != 0, MBR_ONE, 0).astype(i64)
        Dc = np.cumsum(dl, axis=1)
        valid = col[None, :] <= S[:, None]
        a_utt = self.n_utt[self.src]
        starts = first[live]
        is_start = np.zeros(N, bool)
        is_start[starts] = True
        alpha = np.zeros((N, C), i64)
        alpha[starts] = Dc[live]

        def chain(au, w, utt):
            ins = np.where(w != 0, MBR_SUB, 0).astype(i64)[:, None]
            sub = np.where(w[:, None] == R[utt], 0, MBR_SUB).astype(i64)
            A2 = au + ins
            A1 = np.full_like(au, 1 << 60)
            A1[:, 1:] = au[:, :-1] + sub[:, 1:]
            d = Dc[utt]
            return A1, A2, d + np.minimum.accumulate(np.minimum(A1, A2) - d, axis=1)

        def weigh(p, v, utt):
            out = np.rint(p[:, None] * v.astype(np.float64)).astype(i64)
            out[~valid[utt]] = 0
            return out

        groups = []
        for lv, src, _, _ in self.levels:
            keep = live[a_utt[lv]] & ~is_start[self.dst[lv]] & (pi[lv] > 0)
            if keep.any():
                groups.append((lv[keep], src[keep], a_utt[lv[keep]]))
        for lv, src, utt in groups:
            a = chain(alpha[src], self.ol[lv], utt)[2]
            np.add.at(alpha, self.dst[lv], weigh(pi[lv], a, utt))
        ev = np.nonzero((pe > 0) & live[self.n_utt])[0]
        e_utt = self.n_utt[ev]
        no_word = np.zeros(len(ev), i64)
        alpha_e = np.zeros((B, C), i64)
        np.add.at(alpha_e, e_utt, weigh(pe[ev], chain(alpha[ev], no_word, e_utt)[2], e_utt))
        risk = alpha_e[np.arange(B), S]

        beta = np.zeros((N, C), i64)
        flat = beta.reshape(-1)
        beta_e = np.zeros((B, C), i64)
        beta_e[live, S[live]] = MBR_MASS
        k_utt, k_q, k_w, k_g, k_t = [], [], [], [], []

        def note(utt, q, w, g, t):
            k_utt.append(utt), k_q.append(q), k_w.append(w), k_g.append(g), k_t.append(t)

        def back(u, w, utt, p, bv, tv):
            A1, A2, a = chain(alpha[u], w, utt)
            A3 = np.zeros_like(a)
            A3[:, 1:] = a[:, :-1] + dl[utt][:, 1:]
            c1 = (A1 <= A2) & (A1 <= A3)
            c2 = ~c1 & (A2 <= A3)
            c3 = ~c1 & ~c2
            c1[:, 0] = c2[:, 0] = c3[:, 0] = False
            mass = weigh(p, bv, utt)
            n = len(mass)
            # b(q) = mass(q) + (case 3 at q + 1 ? b(q + 1) : 0): suffix sums cut where the chain breaks
            cs = np.zeros((n, C + 1), i64)
            cs[:, :C] = np.cumsum(mass[:, ::-1], axis=1)[:, ::-1]
            brk = np.concatenate([np.where(c3, C, col[None, :]), np.full((n, 1), C)], axis=1)
            nxt = np.minimum.accumulate(brk[:, ::-1], axis=1)[:, ::-1][:, 1:]
            b = cs[:, :C] - np.take_along_axis(cs, nxt, axis=1)
            rows, cols = np.nonzero(b > 0)
            bb = b[rows, cols]
            k1, k2, k3, k0 = c1[rows, cols], c2[rows, cols], c3[rows, cols], cols == 0
            np.add.at(flat, u[rows[k1]] * C + cols[k1] - 1, bb[k1])
            np.add.at(flat, u[rows[k2]] * C + cols[k2], bb[k2])
            np.add.at(flat, u[rows[k0]] * C, bb[k0])
            note(utt[rows[k1]], cols[k1], w[rows[k1]], bb[k1], (bb[k1] >> MBR_TAU_SHIFT) * tv[rows[k1]])
            note(utt[rows[k3]], cols[k3], np.zeros(int(k3.sum()), i64), bb[k3], np.zeros(int(k3.sum()), i64))

        frames = np.array([l.num_frames for l in self.lattices], i64)
        back(ev, no_word, e_utt, pe[ev], beta_e[e_utt], frames[e_utt])
        for lv, src, utt in reversed(groups):
            back(src, self.ol[lv].astype(i64), utt, pi[lv], beta[self.dst[lv]], self.time[self.dst[lv]])
        # the start node: nothing of the lattice is left, the rest of the hypothesis is deleted
        tail = np.where(valid[live], beta[starts], 0)
        tail = np.cumsum(tail[:, ::-1], axis=1)[:, ::-1]
        tail[:, 0] = 0
        rows, cols = np.nonzero(tail > 0)
        note(np.nonzero(live)[0][rows], cols, np.zeros(len(rows), i64), tail[rows, cols], np.zeros(len(rows), i64))
        utt, q, w, g, t = (np.concatenate(x).astype(i64) for x in (k_utt, k_q, k_w, k_g, k_t))
        V = int(max(self.ol.max() if len(self.ol) else 0, 0)) + 1
        key, inv = np.unique((utt * C + q) * V + w, return_inverse=True)
        gs, ts = np.zeros(len(key), i64), np.zeros(len(key), i64)
        np.add.at(gs, inv, g)
        np.add.at(ts, inv, t)
        tables = [{} for _ in range(B)]
        for k, gi, ti in zip(key.tolist(), gs.tolist(), ts.tolist()):
            slot, word = divmod(k, V)
            b, qq = divmod(slot, C)
            tables[b][(qq, word)] = (gi, ti)
        return risk, tables


def mbr_update(words, table):
    """the next hypothesis: every slot takes the word of the largest gamma; among equal maxima the
    slot's current word if it is one of them, else the smallest label; the zeros are dropped"""
    S = 2 * len(words) + 1
    slots = [[] for _ in range(S + 1)]
    for (q, w), (g, _) in table.items():
        if g > 0 and 1 <= q <= S:
            slots[q].append((g, w))
    new = []
    for q in range(1, S + 1):
        if not slots[q]:
            continue
        top = max(g for g, _ in slots[q])
        cands = [w for g, w in slots[q] if g == top]
        cur = words[q // 2 - 1] if q % 2 == 0 else 0
        w = cur if cur in cands else min(cands)
        if w != 0:
            new.append(int(w))
    return new


class LatticePosteriors(object):
    """What LatticeBatch.posteriors and DeviceLatticeBatch.posteriors return.

    log_z [B], arc_log_post [total arcs], node_log_post [total nodes]: fp64, numpy arrays from the
    host path and tensors on the batch's device from the device path; arcs and nodes in the batch's
    order, utterance after utterance.  log_z is -inf for an utterance without a lattice."""

    def __init__(self, batch, log_z, arc_log_post, node_log_post, acoustic_scale, lm_scale):
        self.batch, self.log_z, self.arc_log_post, self.node_log_post = batch, log_z, arc_log_post, node_log_post
        self.acoustic_scale, self.lm_scale = acoustic_scale, lm_scale

    def _host_batch(self):
        b = self.batch
        return b if isinstance(b, LatticeBatch) else LatticeBatch(b.lattices())

    def frame_posteriors(self, num_frames=None, num_classes=None):
        """[T, B, C] float32: entry (k - 1, b, c) is the posterior mass of the emitting arcs of
        utterance b into time k that read class c (ilabel c + 1): the recipe toolchain's
        lattice-to-post.  Zero beyond the utterance's frames.  T defaults to the longest utterance
        (the device batch remembers its log_probs' T), C to the largest class the graph reads."""
        b = self.batch
        if isinstance(b, LatticeBatch):
            lats = b.lattices
            B = len(lats)
            T = max([l.num_frames for l in lats] + [0]) if num_frames is None else int(num_frames)
            C = (b.graph.max_ilabel if B else 0) if num_classes is None else int(num_classes)
            out = torch.zeros((T, B, C), dtype=torch.float32)
            if not B or not len(b.arc):
                return out
            il = torch.from_numpy(b.graph.ilabel[b.arc])
            k = torch.from_numpy(b.time[b.dst])
            utt = torch.from_numpy(b.n_utt[b.src])
            post = torch.from_numpy(np.asarray(self.arc_log_post))
        else:
            B = b.num_utterances
            T = b.max_frames if num_frames is None else int(num_frames)
            C = b.num_classes if num_classes is None else int(num_classes)
            out = torch.zeros((T, B, C), dtype=torch.float32, device=b.device)
            if not B or not b.num_arcs:
                return out
            il = b.ilabel.long()
            k = b.time.long()[b.dst_global]
            utt = b.arc_utt
            post = self.arc_log_post
        em = il > 0
        if bool(((il[em] > C) | (k[em] > T)).any()):
            raise ValueError("frame_posteriors: the lattice has classes or frames beyond [T, B, C] = %s"
                             % (tuple(out.shape),))
        flat = ((k[em] - 1) * B + utt[em]) * C + (il[em] - 1)
        acc = torch.zeros(T * B * C, dtype=torch.float64, device=out.device)
        acc.index_add_(0, flat, torch.exp(post[em]))
        return acc.reshape(T, B, C).float()

    def word_posteriors(self, window=0):
        """Per utterance a list of (word, frame, posterior), one entry for each word-bearing arc of
        the best path at these scales: the summed posterior of the utterance's arcs that carry the
        same word and end within `window` frames of that arc's end time, clipped to 1.  Computed
        on the host.  This is a time-window confidence (how much of the lattice's probability mass
        agrees that the word is spoken there): no edit-distance alignment between paths is made.
        The edit-distance-aligned confidence, Kaldi's MBR confidence, is `mbr(...)`'s: MBRResult's
        `confidence`, the mass gamma of a word's slot (LatticeBatch.mbr, DeviceLatticeBatch.mbr)."""
        hb = self._host_batch()
        _, word_arcs = hb._best_paths(self.acoustic_scale, self.lm_scale)
        post = self.arc_log_post
        post = np.exp(post.cpu().numpy() if isinstance(post, torch.Tensor) else np.asarray(post))
        out = []
        if not hb.lattices or not len(hb.time):
            return [[] for _ in hb.lattices]
        t_end = hb.time[hb.dst]
        a_utt = hb.n_utt[hb.src]
        for b, arcs in enumerate(word_arcs):
            mine = np.nonzero(a_utt == b)[0]
            row = []
            for j in arcs:
                same = mine[(hb.ol[mine] == hb.ol[j]) & (np.abs(t_end[mine] - t_end[j]) <= int(window))]
                row.append((int(hb.ol[j]), int(t_end[j]), float(min(1.0, post[same].sum()))))
            out.append(row)
        return out


def best_paths(lattices, acoustic_scale=None, lm_scale=1.0):
    """Lattice.best_path of many lattices over one graph in one dynamic programme"""
    return LatticeBatch(lattices).best_paths(acoustic_scale, lm_scale)


def _empty(graph, scale, n):
    z = np.zeros(0, np.int32)
    f = np.zeros(0, np.float32)
    return Lattice(graph, scale, n, INF, False, z, z, f, f, z, z, z, f)


# ----------------------------------------------------------------------------------
# host path: numpy float32 arithmetic, the same operations as the kernel
# ----------------------------------------------------------------------------------
def _min_at(beta, owner, q):
    ok = q < INF
    np.minimum.at(beta, owner[ok], q[ok])


def _host_one(g, lp, n, beam, lattice_beam, scale, allow_partial, cost, arcof):
    """one utterance: lp [T, C] float32; cost / arcof as in wfst_decode._host_one.
    Returns (Lattice, stats)."""
    stats = dict(peak_emit=0, peak_closure=0, records=0, nodes=0, arcs=0)
    T = lp.shape[0]
    if n < 1 or n > T:
        return _empty(g, scale, n), stats
    beam, f_scale, zero = np.float32(beam), np.float32(scale), np.float32(0)
    cost[g.start], arcof[g.start] = 0.0, _NOARC
    act = np.array([g.start], np.int64)
    frames, thr = [], [np.float32(np.nan)]
    cur_s = cur_c = None
    for t in range(-1, n):
        if t >= 0:
            a_sc = -(f_scale * lp[t])
            arcs, owner = _ranges(g.ptr[cur_s], g.ptr[cur_s + 1])
            em = g.ilabel[arcs] > 0
            arcs, owner = arcs[em], owner[em]
            c = (cur_c[owner] + g.weight[arcs]) + a_sc[g.ilabel[arcs] - 1]
            act = _merge(g, cost, arcof, np.zeros(0, np.int64), arcs, c)
            stats['peak_emit'] = max(stats['peak_emit'], len(act))
            th = np.float32(cost[act].min() + beam) if len(act) else np.float32(np.nan)
            thr.append(th)
            drop = act[~(cost[act] <= th)]
            cost[drop] = INF
            arcof[drop] = _NOARC
            act = act[cost[act] <= th]
        act = _closure(g, cost, arcof, act)
        stats['peak_closure'] = max(stats['peak_closure'], len(act))
        stats['records'] += len(act)
        V = np.sort(act)
        al, ar = cost[V].copy(), arcof[V].copy()
        surv = al <= al.min() + beam if (t < n - 1 and len(V)) else np.ones(len(V), bool)
        frames.append((V, al, ar, surv))
        cur_s, cur_c = V[surv], al[surv]
        cost[act] = INF
        arcof[act] = _NOARC
    V, al, _, _ = frames[n]
    if not len(V):
        return _empty(g, scale, n), stats
    tot = (al + g.final[V]) + zero
    ok = tot < INF
    reached = bool(ok.any())
    if reached:
        best = tot[ok].min()
        s = int(V[ok][tot[ok] == best].min())
    elif allow_partial:
        best = al.min()
        s = int(V[al == best].min())
    else:
        return _empty(g, scale, n), stats
    # the arcs of the search's own traceback, by the time of their source
    forced = [[] for _ in range(n + 1)]
    k = n
    while True:
        Vk, _, ark, _ = frames[k]
        a = int(ark[np.searchsorted(Vk, s)])
        if a == _NOARC:
            break
        if g.ilabel[a] > 0:
            k -= 1
        forced[k].append(a)
        s = int(g.src[a])
    limit = np.float32(best) + np.float32(lattice_beam)
    betas = [None] * (n + 1)
    base = np.cumsum([0] + [len(f[0]) for f in frames])
    k_src, k_dst, k_arc, k_lp = [], [], [], []

    def keep(k, owner, kd, pos, arcs, q, alpha, scores):
        val = alpha[owner] + q
        m = ((val < INF) & (val <= limit)) | np.isin(arcs, forced[k])
        k_src.append(base[k] + owner[m])
        k_dst.append(base[kd] + pos[m])
        k_arc.append(arcs[m])
        k_lp.append(scores[m] if scores is not None else np.zeros(int(m.sum()), np.float32))

    for k in range(n, -1, -1):
        V, al, _, surv = frames[k]
        if k == n:
            beta = (g.final[V] + zero) if reached else np.zeros(len(V), np.float32)
        else:
            beta = np.full(len(V), INF, np.float32)
            Vn = frames[k + 1][0]
            a_sc = -(f_scale * lp[k])
            idx = np.nonzero(surv)[0]
            arcs, owner = _ranges(g.ptr[V[idx]], g.ptr[V[idx] + 1])
            owner = idx[owner]
            em = g.ilabel[arcs] > 0
            arcs, owner = arcs[em], owner[em]
            cls = g.ilabel[arcs] - 1
            p = ((al[owner] + g.weight[arcs]) + a_sc[cls]) + zero
            m = (p < INF) & (p <= thr[k + 1])
            arcs, owner, cls = arcs[m], owner[m], cls[m]
            pos = np.searchsorted(Vn, g.dst[arcs])
            q = ((g.weight[arcs] + a_sc[cls]) + betas[k + 1][pos]) + zero
            _min_at(beta, owner, q)
            keep(k, owner, k + 1, pos, arcs, q, al, lp[k][cls])
        for r in range(g.num_ranks - 1, -1, -1):
            idx = np.nonzero((g.rank[V] == r) & (g.eps_ptr[V + 1] > g.eps_ptr[V]))[0]
            if not len(idx):
                continue
            e, owner = _ranges(g.eps_ptr[V[idx]], g.eps_ptr[V[idx] + 1])
            owner = idx[owner]
            arcs = g.eps_arc[e]
            d = g.dst[arcs]
            pos = np.minimum(np.searchsorted(V, d), len(V) - 1)
            m = (V[pos] == d) & (((al[owner] + g.weight[arcs]) + zero) < INF)
            arcs, owner, pos = arcs[m], owner[m], pos[m]
            q = (g.weight[arcs] + beta[pos]) + zero
            _min_at(beta, owner, q)
            keep(k, owner, k, pos, arcs, q, al, None)
        betas[k] = beta
    src = np.concatenate(k_src).astype(np.int64)
    dst = np.concatenate(k_dst).astype(np.int64)
    arc = np.concatenate(k_arc).astype(np.int64)
    alp = np.concatenate(k_lp).astype(np.float32)
    used = np.zeros(base[-1], bool)
    used[src] = True
    used[dst] = True
    used[base[0] + np.searchsorted(frames[0][0], g.start)] = True
    new_id = np.cumsum(used) - 1                   # records are ordered by (time, state) already
    order = np.lexsort((arc, new_id[src]))
    times = np.repeat(np.arange(n + 1), [len(f[0]) for f in frames])
    stats['nodes'], stats['arcs'] = int(used.sum()), len(arc)
    lat = Lattice(g, scale, n, best, reached, times[used], np.concatenate([f[0] for f in frames])[used],
                  np.concatenate([f[1] for f in frames])[used], np.concatenate(betas)[used],
                  new_id[src][order], new_id[dst][order], arc[order], alp[order])
    return lat, stats


def decode_lattice_host(lp, lens, graph, beam=16.0, lattice_beam=8.0, acoustic_scale=1.0, allow_partial=True):
    """The host path on numpy arrays: lp [T,B,C] float32.  Returns (lattices, stats): per utterance
    what a device run needs of its capacities (peak_emit / peak_closure against list_cap, records
    against log_cap, nodes against node_cap, arcs against arc_cap)."""
    lp = np.asarray(lp, np.float32)
    B = lp.shape[1]
    cost = np.full(graph.num_states, INF, np.float32)
    arcof = np.full(graph.num_states, _NOARC, np.int64)
    lats, stats = [], []
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(B):
            lat, st = _host_one(graph, lp[:, b], int(lens[b]), beam, lattice_beam, acoustic_scale,
                                allow_partial, cost, arcof)
            lats.append(lat)
            stats.append(st)
    return lats, stats


# ----------------------------------------------------------------------------------
# device path
# ----------------------------------------------------------------------------------
def plan_workspace(num_states, T, B, workspace_bytes, num_arcs=None):
    """(utterances per launch, list_cap, log_cap, node_cap, arc_cap) for a workspace budget.

    wfst_decode.plan_workspace's scheme with the lattice's sizes: a record of the log takes 24 bytes
    (arc, source record, state, alpha, beta, marks) where the 1-best search takes 8, and per
    utterance there are 8 (T + 2) bytes of per-time offsets and thresholds.  The budget also
    covers what comes back: 16 bytes a kept node, 16 bytes a kept arc.  When it holds a quarter of
    the batch at the sizes that cannot overflow (a node per state and time, every graph arc at
    every time; num_arcs None: four arcs a state) that is the plan.  Otherwise a quarter of the
    budget is set aside for nodes and arcs, one node to four arcs, and the rest is planned as for
    the 1-best search.  node_cap never needs to exceed log_cap."""
    tables = 12 * num_states + 8 * (T + 2)
    if workspace_bytes < tables + 20 + 24 + 16 + 16 + 64:
        raise ValueError("workspace_bytes = %d cannot hold one utterance's tables (%d bytes)"
                         % (workspace_bytes, tables + 140))
    rec = (T + 1) * num_states
    arcs = max(1, (T + 1) * (4 * num_states if num_arcs is None else num_arcs))
    full = tables + 20 * num_states + (24 + 16) * rec + 16 * arcs + 64
    if 4 * (workspace_bytes // full) >= B and max(rec, arcs) < 2 ** 31 - 1:
        return int(min(B, workspace_bytes // full)), int(num_states), int(rec), int(rec), int(arcs)
    search = workspace_bytes - workspace_bytes // 4
    chunk = B if B * tables <= search // 2 else max(1, (search // 2) // tables)
    chunk = max(1, min(chunk, B, workspace_bytes // (tables + 20 + 24 + 32 + 64)))
    rest = search // chunk - tables - 64
    list_cap = int(min(num_states, max(1, rest // 4 // 20), 2 ** 31 - 2))
    log_cap = int(min((T + 1) * list_cap, max(1, (rest - 20 * list_cap) // 24), 2 ** 31 - 2))
    out = (workspace_bytes // 4) // chunk
    node_cap = int(min(log_cap, max(1, out // 5 // 16)))
    arc_cap = int(min(2 ** 31 - 2, max(1, (out - 16 * node_cap) // 16)))
    return chunk, list_cap, log_cap, node_cap, arc_cap


THREADS_PER_WORKGROUP = 0       # 0: the kernel's default; 256 / 512 / 1024 for timing runs


def _decode_device(lp, lens, graph, beam, lattice_beam, scale, allow_partial, workspace_bytes, pack=True,
                   to_host=True):
    """launches asr_wfst_lattice_f32; returns per-utterance counts and the kept nodes and arcs of the
    whole batch, packed utterance after utterance and already in canonical order, as numpy arrays:
    only those cross to the host.  pack=False (tools/bench_wfst_lattice.py): the launches alone.
    to_host=False (att_speech.lattice_dp.decode_lattice_device): the same as device tensors, nothing
    is copied."""
    T, B, C = lp.shape
    L = _native.lib()
    g = graph
    if not L.asr_wfst_lattice_supported(g.num_states, len(g.src), C, T):
        raise NotImplementedError(
            "asr_wfst_lattice_f32 serves 1 <= C <= 4096 classes and T >= 1 (got C = %d, T = %d); "
            "ASR_WFST_LATTICE_NATIVE=0 selects the host path" % (C, T))
    dev = lp.device
    d = g.device_arrays(dev)
    lens_d = torch.as_tensor(np.asarray(lens, np.int32)).to(dev)
    chunk, list_cap, log_cap, node_cap, arc_cap = plan_workspace(g.num_states, T, B, workspace_bytes, len(g.src))
    nbytes = L.asr_wfst_lattice_workspace_bytes(g.num_states, chunk, T, list_cap, log_cap)
    if not 0 < nbytes:
        raise ValueError("workspace_bytes = %d is too small" % workspace_bytes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    cost = torch.empty(B, **f32)
    final, overflow, n_nodes, n_arcs = (torch.empty(B, **i32) for _ in range(4))
    p = _native._p
    packed = [[] for _ in range(8)]
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        nb = b1 - b0
        node_i = torch.empty((2, nb, node_cap), **i32)      # time, state
        node_f = torch.empty((2, nb, node_cap), **f32)      # alpha, beta
        arc_i = torch.empty((3, nb, arc_cap), **i32)        # src, dst, arc
        arc_f = torch.empty((nb, arc_cap), **f32)           # lp
        _native.check(L.asr_wfst_lattice_f32(
            p(lp[:, b0]), B * C, p(lens_d[b0:]), T, nb, C, g.num_states, len(g.src),
            p(d['ptr']), p(d['src']), p(d['dst']), p(d['il']), p(d['ol']), p(d['w']), p(d['fin']),
            p(d['eps_ptr']), p(d['eps_arc']), len(g.eps_arc), p(d['rank']), g.num_ranks, g.start,
            float(beam), float(lattice_beam), float(scale), int(bool(allow_partial)),
            list_cap, log_cap, node_cap, arc_cap, int(THREADS_PER_WORKGROUP),
            p(cost[b0:]), p(final[b0:]), p(n_nodes[b0:]), p(n_arcs[b0:]),
            p(node_i[0]), p(node_i[1]), p(node_f[0]), p(node_f[1]),
            p(arc_i[0]), p(arc_i[1]), p(arc_i[2]), p(arc_f), p(overflow[b0:]),
            p(ws), nbytes, _native._stream()), 'asr_wfst_lattice_f32')
        if not pack:
            continue
        ok = overflow[b0:b1] == 0
        rows = torch.arange(nb, device=dev)

        def used(count, cap):
            """flat indices of the first count[b] slots of every row of a [nb, cap] array, and the rows"""
            count = torch.where(ok, count, torch.zeros_like(count)).long()
            total = int(count.sum())                # the one read-back the packing needs
            r = torch.repeat_interleave(rows, count, output_size=total)
            first = torch.cumsum(count, 0) - count
            return r * cap + (torch.arange(total, device=dev) - first[r]), r, first
        ni, n_utt, n_first = used(n_nodes[b0:b1], node_cap)
        ai, a_utt, _ = used(n_arcs[b0:b1], arc_cap)
        time, state = node_i[0].reshape(-1)[ni].long(), node_i[1].reshape(-1)[ni].long()
        # canonical order, here where sorting is cheap: nodes by (utterance, time, state) ...
        order = _order((n_utt, time, state), (nb, T + 1, g.num_states))
        rank = torch.empty_like(order)
        rank[order] = torch.arange(len(order), device=dev)
        # ... arcs by (utterance, src node, graph arc index); src / dst renumbered within the utterance
        src = rank[arc_i[0].reshape(-1)[ai].long() + n_first[a_utt]]
        dst = rank[arc_i[1].reshape(-1)[ai].long() + n_first[a_utt]]
        arc = arc_i[2].reshape(-1)[ai].long() & 0xFFFFFFFF
        ao = _order((src, arc), (max(1, len(order)), max(1, len(g.src))))        # src is global: utterance-major
        for j, t in enumerate((time[order].int(), state[order].int(), node_f[0].reshape(-1)[ni][order],
                               node_f[1].reshape(-1)[ni][order], (src - n_first[a_utt])[ao].int(),
                               (dst - n_first[a_utt])[ao].int(), arc[ao], arc_f.reshape(-1)[ai][ao])):
            packed[j].append(t)
    if not pack:
        return None
    packed = [torch.cat(x) for x in packed]
    if not to_host:
        return cost, final, n_nodes, n_arcs, overflow, packed
    return (cost.cpu().numpy(), final.cpu().numpy(), n_nodes.cpu().numpy(), n_arcs.cpu().numpy(),
            overflow.cpu().numpy(), [x.cpu().numpy() for x in packed])


def _order(keys, bounds):
    """argsort of rows by `keys` (int64 tensors, most significant first, 0 <= key < bound): one sort
    of a composite key when it fits 62 bits, else stable sorts from the least significant key up"""
    span = 1
    for b in bounds:
        span *= int(b)
    if span < 2 ** 62:
        key = keys[0]
        for k, b in zip(keys[1:], bounds[1:]):
            key = key * int(b) + k
        return torch.sort(key)[1]
    order = torch.sort(keys[-1], stable=True)[1]
    for k in reversed(keys[:-1]):
        order = order[torch.sort(k[order], stable=True)[1]]
    return order


def _validate(log_probs, lens, graph, beam, lattice_beam):
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
    if not (float(lattice_beam) >= 0.0):
        raise ValueError("lattice_beam must be >= 0")
    lens_np = np.asarray(torch.as_tensor(lens).cpu(), np.int64).reshape(-1)
    if len(lens_np) != B:
        raise ValueError("lens must have one entry per utterance")
    if len(lens_np) and (lens_np.min() < 1 or lens_np.max() > T):
        raise ValueError("lens must lie in [1, T]")
    lp = log_probs.detach()
    if lp.dtype != torch.float32:
        lp = lp.float()
    return lp, lens_np


def decode_lattice(log_probs, lens, graph, beam=16.0, lattice_beam=8.0, acoustic_scale=1.0,
                   allow_partial=True, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """One search per utterance, one `Lattice` per utterance: (lattices, redone_on_host).

    Arguments as decode_graph, plus lattice_beam >= 0 (+inf: every arc the search saw that lies on
    a complete path).  A GPU tensor runs asr_wfst_lattice_f32; a CPU tensor, or
    ASR_WFST_LATTICE_NATIVE=0 (read per call), the host path, which gives the same bits.  An
    utterance that outgrows the device's token lists, its log, or the node or arc capacity
    (plan_workspace) is redone on the host, with one warning per call."""
    lp, lens_np = _validate(log_probs, lens, graph, beam, lattice_beam)
    T, B, C = lp.shape
    native = lp.is_cuda and os.environ.get('ASR_WFST_LATTICE_NATIVE', '1') != '0'
    if not native or B == 0 or T == 0:
        lats, _ = decode_lattice_host(lp.cpu().numpy(), lens_np, graph, beam, lattice_beam, acoustic_scale,
                                      allow_partial)
        return lats, []
    lp = lp.contiguous()
    cost, final, n_nodes, n_arcs, overflow, packed = _decode_device(
        lp, lens_np, graph, beam, lattice_beam, acoustic_scale, allow_partial, int(workspace_bytes))
    redo = np.nonzero(overflow)[0].tolist()
    n_nodes = np.where(overflow != 0, 0, n_nodes)
    n_arcs = np.where(overflow != 0, 0, n_arcs)
    no = np.r_[0, np.cumsum(n_nodes)]
    ao = np.r_[0, np.cumsum(n_arcs)]
    lats = []
    for b in range(B):
        ns, as_ = slice(no[b], no[b + 1]), slice(ao[b], ao[b + 1])
        if overflow[b] or n_nodes[b] == 0:
            lats.append(_empty(graph, acoustic_scale, lens_np[b]))
            continue
        lats.append(Lattice(graph, acoustic_scale, lens_np[b], cost[b], final[b] != 0,
                            *[x[ns] for x in packed[:4]], *[x[as_] for x in packed[4:]]))
    if redo:
        warnings.warn("decode_lattice: %d of %d utterances outgrew the device workspace (%s; "
                      "workspace_bytes = %d) and were decoded on the host"
                      % (len(redo), B, ', '.join(sorted({OVERFLOW_NAMES.get(int(overflow[b]), '?') for b in redo})),
                         workspace_bytes))
        idx = torch.as_tensor(redo, device=lp.device)
        h, _ = decode_lattice_host(lp[:, idx].cpu().numpy(), lens_np[redo], graph, beam, lattice_beam,
                                   acoustic_scale, allow_partial)
        for j, b in enumerate(redo):
            lats[b] = h[j]
    return lats, redo
