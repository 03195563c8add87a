"""An independent referee of att_speech.wfst_decode's semantics, in fp64
numpy: dense over ALL states of the graph at every frame, no active lists, no shared code with
the product (it takes the arc arrays in arc-index order and ranks the epsilon arcs itself).
Plus a brute-force enumerator of all paths for toy graphs.

Minima and ties are found with np.minimum.at over all arcs at once: first the cost of every
destination, then, among the arcs that attain it, the smallest arc index."""
import numpy as np

INF = float('inf')
NOARC = np.int64(2 ** 40)


def eps_ranks(num_states, src, dst, ilabel):
    """rank[s] = longest epsilon path ending in s, by relaxation (None: a cycle)"""
    e = np.nonzero(np.asarray(ilabel) == 0)[0]
    rank = np.zeros(num_states, np.int64)
    for _ in range(num_states + 1):
        new = rank.copy()
        np.maximum.at(new, dst[e], rank[src[e]] + 1)
        if (new == rank).all():
            return rank
        rank = new
    return None


def _relax(cost, bp, arcs, dst, cand):
    """min-merge the proposals (arcs, cand) into (cost, bp), smallest arc index among equal costs"""
    ok = np.isfinite(cand)
    arcs, dst, cand = arcs[ok], dst[ok], cand[ok]
    best = cost.copy()
    np.minimum.at(best, dst, cand)
    bp[best < cost] = NOARC
    cost[:] = best
    win = cand == cost[dst]
    np.minimum.at(bp, dst[win], arcs[win])


def _prune(cost, bp, beam):
    fin = np.isfinite(cost)
    if fin.any():
        drop = fin & ~(cost <= cost[fin].min() + beam)
        cost[drop] = INF
        bp[drop] = NOARC


def decode(num_states, start, src, dst, ilabel, olabel, weight, final, lp, lens, beam=16.0,
           acoustic_scale=1.0, allow_partial=True):
    """lp [T,B,C]; the arc arrays in arc-index order.  Returns the fields of decode_graph as numpy
    arrays / lists (cost as float64)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    il, ol = np.asarray(ilabel, np.int64), np.asarray(olabel, np.int64)
    w, final = np.asarray(weight, np.float64), np.asarray(final, np.float64)
    lp = np.asarray(lp, np.float64)
    T, B, _ = lp.shape
    rank = eps_ranks(num_states, src, dst, il)
    assert rank is not None, "epsilon cycle"
    arcs = np.arange(len(src), dtype=np.int64)
    em = arcs[il > 0]
    eps = arcs[il == 0]
    levels = [eps[rank[src[eps]] == r] for r in range(int(rank[src[eps]].max()) + 1)] if len(eps) else []
    out = dict(words=[], alignment=np.full((B, T), -1, np.int32), cost=np.full(B, INF),
               reached_final=np.zeros(B, bool), num_active=np.zeros((B, T), np.int32),
               abs_terms=np.zeros(B))        # sum of |term| over the terms of the best path's cost

    def closure(cost, bp):
        for lv in levels:
            _relax(cost, bp, lv, dst[lv], cost[src[lv]] + w[lv])

    for b in range(B):
        n = int(lens[b])
        cost = np.full(num_states, INF)
        bp = np.full(num_states, NOARC, np.int64)
        cost[start] = 0.0
        closure(cost, bp)
        logs = [bp.copy()]
        if n > 0:
            _prune(cost, bp, beam)
        for t in range(n):
            a = -(acoustic_scale * lp[t, b])
            ncost = np.full(num_states, INF)
            nbp = np.full(num_states, NOARC, np.int64)
            _relax(ncost, nbp, em, dst[em], (cost[src[em]] + w[em]) + a[il[em] - 1])
            _prune(ncost, nbp, beam)
            closure(ncost, nbp)
            logs.append(nbp.copy())
            if t < n - 1:
                _prune(ncost, nbp, beam)
            cost, bp = ncost, nbp
            out['num_active'][b, t] = int(np.isfinite(cost).sum())
        tot = cost + final
        if n < 1:
            out['words'].append([])
            continue
        if np.isfinite(tot).any():
            s = int(np.argmin(tot))                 # first minimum = smallest state id
            best, reached = tot[s], True
        elif allow_partial and np.isfinite(cost).any():
            s = int(np.argmin(cost))
            best, reached = cost[s], False
        else:
            out['words'].append([])
            continue
        words, k, t = [], n, n - 1
        out['abs_terms'][b] = abs(final[s]) if reached else 0.0
        while logs[k][s] != NOARC:
            arc = int(logs[k][s])
            out['abs_terms'][b] += abs(w[arc])
            if il[arc] > 0:
                out['abs_terms'][b] += abs(acoustic_scale * lp[t, b, il[arc] - 1])
                out['alignment'][b, t] = il[arc]
                t -= 1
                k -= 1
            if ol[arc] != 0:
                words.append(int(ol[arc]))
            s = int(src[arc])
        assert t == -1 and s == start
        out['words'].append(words[::-1])
        out['cost'][b], out['reached_final'][b] = best, reached
    return out


def enumerate_paths(num_states, start, src, dst, ilabel, olabel, weight, final, lp, n, acoustic_scale=1.0):
    """Every path from the start state that consumes exactly n frames of lp [T,C] (toy graphs only).
    Returns a list of (cost with the final cost, cost without, tuple of arc indices, end state)."""
    lp = np.asarray(lp, np.float64)
    out_arcs = [[] for _ in range(num_states)]
    for a in range(len(src)):
        out_arcs[int(src[a])].append(a)
    paths = []

    def walk(s, t, c, arcs):
        if t == n:
            paths.append((c + float(final[s]), c, tuple(arcs), s))
        for a in out_arcs[s]:
            if ilabel[a] == 0:
                walk(int(dst[a]), t, c + float(weight[a]), arcs + [a])
            elif t < n:
                walk(int(dst[a]), t + 1, c + float(weight[a]) - acoustic_scale * lp[t, int(ilabel[a]) - 1],
                     arcs + [a])

    walk(start, 0, 0.0, [])
    return paths


def best_other_words_cost(num_states, start, src, dst, ilabel, olabel, weight, final, lp, n, words,
                           acoustic_scale=1.0):
    """The cost of the best path whose word sequence is NOT `words`, for a graph without epsilon
    arcs: dense Viterbi over (state, j) where j counts the words of `words` matched so far and
    one more column holds every path that has left it.  lp [T,C]."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    il, ol = np.asarray(ilabel, np.int64), np.asarray(olabel, np.int64)
    assert (il > 0).all()
    w, final = np.asarray(weight, np.float64), np.asarray(final, np.float64)
    lp = np.asarray(lp, np.float64)
    L = len(words)
    y = np.asarray(list(words) + [-1], np.int64)
    j = np.arange(L + 2)
    # column reached from column j over an arc with output o
    nxt = np.where(ol[:, None] == 0, j[None, :],
                   np.where((j[None, :] < L) & (ol[:, None] == y[np.minimum(j, L)][None, :]), j[None, :] + 1, L + 1))
    nxt[:, L + 1] = L + 1
    cost = np.full((num_states, L + 2), INF)
    cost[start, 0] = 0.0
    rows = np.broadcast_to(dst[:, None], nxt.shape)
    for t in range(n):
        a = -(acoustic_scale * lp[t])
        cand = cost[src] + (w + a[il - 1])[:, None]
        new = np.full_like(cost, INF)
        np.minimum.at(new, (rows, nxt), cand)
        cost = new
    tot = cost + final[:, None]
    tot[:, L] = INF
    return float(tot.min())


def graph_args(g):
    """the arrays of a DecodingGraph, in the order decode() takes them"""
    return (g.num_states, g.start, g.src, g.dst, g.ilabel, g.olabel, g.weight, g.final)
