"""An independent referee of att_speech.wfst_lattice's semantics, in fp64
numpy: dense over ALL states of the graph at every time, minima with np.minimum.at, no active
lists and no code shared with the product.  The forward restates section 4.19 as
tests/wfst_referee.py does, keeping what the lattice needs of every time; brute force goes through
wfst_referee.enumerate_paths."""
import numpy as np

from wfst_referee import NOARC, _prune, _relax, enumerate_paths, eps_ranks

INF = float('inf')
FIELDS = ('time', 'state', 'alpha', 'beta', 'src', 'dst', 'arc', 'lp')


def _empty():
    return dict(cost=INF, reached_final=False, time=np.zeros(0, np.int64), state=np.zeros(0, np.int64),
                alpha=np.zeros(0), beta=np.zeros(0), src=np.zeros(0, np.int64), dst=np.zeros(0, np.int64),
                arc=np.zeros(0, np.int64), lp=np.zeros(0))


def lattice_one(num_states, start, src, dst, ilabel, olabel, weight, final, lp, n, beam=16.0, lattice_beam=8.0,
                acoustic_scale=1.0, allow_partial=True):
    """lp [T,C]; the arc arrays in arc-index order.  Returns the canonical arrays as a dict (costs
    as float64), plus cost and reached_final."""
    N = num_states
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    il = np.asarray(ilabel, np.int64)
    w, final = np.asarray(weight, np.float64), np.asarray(final, np.float64)
    lp = np.asarray(lp, np.float64)
    rank = eps_ranks(N, src, dst, il)
    arcs = np.arange(len(src), dtype=np.int64)
    em, eps = arcs[il > 0], arcs[il == 0]
    levels = [eps[rank[src[eps]] == r] for r in range(int(rank[src[eps]].max()) + 1)] if len(eps) else []

    def closure(cost, bp):
        for lv in levels:
            _relax(cost, bp, lv, dst[lv], cost[src[lv]] + w[lv])

    # forward: alpha[k] over V_k (inf elsewhere), surv[k] = S_k, thr[k], bp[k]
    cost = np.full(N, INF)
    bp = np.full(N, NOARC, np.int64)
    cost[start] = 0.0
    closure(cost, bp)
    alpha, back, surv, thr, a_of = [cost.copy()], [bp.copy()], [], [np.nan], [None]
    _prune(cost, bp, beam)
    surv.append(np.isfinite(cost))
    for t in range(n):
        a = -(acoustic_scale * lp[t])
        a_of.append(a)
        ncost = np.full(N, INF)
        nbp = np.full(N, NOARC, np.int64)
        _relax(ncost, nbp, em, dst[em], (cost[src[em]] + w[em]) + a[il[em] - 1])
        thr.append(ncost[np.isfinite(ncost)].min() + beam if np.isfinite(ncost).any() else np.nan)
        _prune(ncost, nbp, beam)
        closure(ncost, nbp)
        alpha.append(ncost.copy())
        back.append(nbp.copy())
        if t < n - 1:
            _prune(ncost, nbp, beam)
        surv.append(np.isfinite(ncost))
        cost = ncost
    tot = alpha[n] + final
    if np.isfinite(tot).any():
        s_end, reached = int(np.argmin(tot)), True
        best = tot[s_end]
        beta = np.where(np.isfinite(alpha[n]), final, INF)
    elif allow_partial and np.isfinite(alpha[n]).any():
        s_end, reached = int(np.argmin(alpha[n])), False
        best = alpha[n][s_end]
        beta = np.where(np.isfinite(alpha[n]), 0.0, INF)
    else:
        return _empty()
    forced = set()
    k, s = n, s_end
    while back[k][s] != NOARC:
        arc = int(back[k][s])
        if il[arc] > 0:
            k -= 1
        forced.add((k, arc))
        s = int(src[arc])
    assert k == 0 and s == start
    forced_at = [np.array([e for kk, e in forced if kk == k], np.int64) for k in range(n + 1)]

    limit = best + lattice_beam
    kept = []                       # (time of the source, arc)
    betas = [None] * (n + 1)
    for k in range(n, -1, -1):
        al = alpha[k]
        if k < n:
            a = a_of[k + 1]
            p = (al[src[em]] + w[em]) + a[il[em] - 1]
            ok = surv[k][src[em]] & np.isfinite(p) & (p <= thr[k + 1])
            la = em[ok]
            assert (alpha[k + 1][dst[la]] <= p[ok]).all()       # the destination exists and costs no more
            x = w[la] + a[il[la] - 1]
            q = x + betas[k + 1][dst[la]]
            beta = np.full(N, INF)
            np.minimum.at(beta, src[la], q)
            val = al[src[la]] + q
            for j in np.nonzero((np.isfinite(val) & (val <= limit)) | np.isin(la, forced_at[k]))[0]:
                kept.append((k, int(la[j])))
        for lv in reversed(levels):
            ok = np.isfinite(al[src[lv]]) & np.isfinite(al[dst[lv]]) & np.isfinite(al[src[lv]] + w[lv])
            la = lv[ok]
            q = w[la] + beta[dst[la]]
            np.minimum.at(beta, src[la], q)
            val = al[src[la]] + q
            for j in np.nonzero((np.isfinite(val) & (val <= limit)) | np.isin(la, forced_at[k]))[0]:
                kept.append((k, int(la[j])))
        betas[k] = beta
    nodes = {(0, start)}
    for k, e in kept:
        nodes.add((k, int(src[e])))
        nodes.add((k + (1 if il[e] > 0 else 0), int(dst[e])))
    nodes = sorted(nodes)
    index = {v: i for i, v in enumerate(nodes)}
    rows = sorted((index[(k, int(src[e]))], e, index[(k + (1 if il[e] > 0 else 0), int(dst[e]))],
                   lp[k, il[e] - 1] if il[e] > 0 else 0.0) for k, e in kept)
    return dict(cost=best, reached_final=reached,
                time=np.array([v[0] for v in nodes], np.int64), state=np.array([v[1] for v in nodes], np.int64),
                alpha=np.array([alpha[k][s] for k, s in nodes]), beta=np.array([betas[k][s] for k, s in nodes]),
                src=np.array([r[0] for r in rows], np.int64), dst=np.array([r[2] for r in rows], np.int64),
                arc=np.array([r[1] for r in rows], np.int64), lp=np.array([r[3] for r in rows], np.float64))


def lattices(graph_args, lp, lens, **kw):
    """lp [T,B,C]: one dict per utterance"""
    return [lattice_one(*graph_args, lp[:, b], int(lens[b]), **kw) for b in range(lp.shape[1])]


def assert_same(got, want, what=''):
    """a product Lattice against a referee dict: every canonical field, costs compared as numbers
    with == (fp32 against fp64 is exact on the grid)"""
    assert float(got.cost) == float(want['cost']), (what, got.cost, want['cost'])
    assert bool(got.reached_final) == bool(want['reached_final']), what
    for k in FIELDS:
        g, w = np.asarray(getattr(got, k)), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert (g.astype(np.float64) == w.astype(np.float64)).all(), (what, k, g, w)


def paths_within(graph_args, lp, n, lattice_beam, acoustic_scale=1.0, allow_partial=True):
    """Brute force: (best cost, the paths within lattice_beam of it) as [(cost, arcs, words)].
    When no path ends in a final state (allow_partial) costs are those without the final cost."""
    olabel = np.asarray(graph_args[5])
    paths = enumerate_paths(*graph_args, lp, n, acoustic_scale)
    if any(np.isfinite(p[0]) for p in paths):
        cand = [(p[0], p[2]) for p in paths if np.isfinite(p[0])]
    elif allow_partial:
        cand = [(p[1], p[2]) for p in paths if np.isfinite(p[1])]
    else:
        cand = []
    if not cand:
        return INF, []
    best = min(c for c, _ in cand)
    return best, [(c, arcs, [int(olabel[a]) for a in arcs if olabel[a] != 0])
                  for c, arcs in cand if c <= best + lattice_beam]


def nbest_of(paths, n):
    """the n cheapest distinct word sequences of brute-force paths, by (cost, words)"""
    cheapest = {}
    for c, _, words in paths:
        key = tuple(words)
        cheapest[key] = min(c, cheapest.get(key, INF))
    return sorted(((list(k), c) for k, c in cheapest.items()), key=lambda e: (e[1], e[0]))[:n]
