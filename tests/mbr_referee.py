"""Referee of minimum-Bayes-risk decoding over lattices (LatticeBatch.mbr, asr_lattice_mbr_f64).  Shares
no code with the implementation:

  (a) `evaluate`: the semantics of include/asr_amd.h, one lattice and one given hypothesis, in plain
      Python floats, node by node and slot by slot;
  (b) `expected_edit_distance`: the sum over every complete path of P(path) * Levenshtein(words(path),
      hypothesis), paths from lattice_dp_referee.scored_paths.
"""
import math

from lattice_dp_referee import INF, _arc_cost, _end_cost, _scales, scored_paths

DELTA = 1e-5


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def expected_edit_distance(lat, hyp, acoustic_scale=None, lm_scale=1.0):
    paths = scored_paths(lat, acoustic_scale, lm_scale)
    paths = [p for p in paths if p['cost'] < INF]
    if not paths:
        return INF
    low = min(p['cost'] for p in paths)
    weights = [math.exp(low - p['cost']) for p in paths]
    z = math.fsum(weights)
    return math.fsum(w / z * levenshtein(p['words'], list(hyp)) for w, p in zip(weights, paths))


def _log_add(values):
    values = [v for v in values if v > -INF]
    if not values:
        return -INF
    m = max(values)
    return m + math.log(math.fsum(math.exp(v - m) for v in values))


def _topological(lat):
    """node indices such that every arc leads forwards: by (time, epsilon rank of the state)"""
    rank = lat.graph.rank
    return sorted(range(lat.num_nodes), key=lambda v: (int(lat.time[v]), int(rank[int(lat.state[v])]), v))


def evaluate(lat, hyp, acoustic_scale=None, lm_scale=1.0):
    """(risk, gamma): gamma[q] = {word: mass} for the slots q = 1 .. 2 len(hyp) + 1"""
    sc, lm = _scales(lat, acoustic_scale, lm_scale)
    n = lat.num_nodes
    order = _topological(lat)
    starts = [v for v in range(n) if lat.time[v] == 0 and lat.state[v] == lat.graph.start]
    if not starts:
        return INF, None
    s = starts[0]
    into = [[] for _ in range(n)]
    for j in range(lat.num_arcs):
        into[int(lat.dst[j])].append(j)
    word = [int(lat.graph.olabel[int(lat.arc[j])]) for j in range(lat.num_arcs)]
    x = [_arc_cost(lat, j, sc, lm) for j in range(lat.num_arcs)]
    fwd = [-INF] * n
    fwd[s] = 0.0
    for v in order:
        if v != s:
            fwd[v] = _log_add([fwd[int(lat.src[j])] - x[j] for j in into[v] if x[j] < INF])
    stops = {}
    for v in range(n):
        e = _end_cost(lat, v)
        if e is not None and fwd[v] > -INF:
            stops[v] = fwd[v] - lm * e
    log_z = _log_add(list(stops.values()))
    if log_z == -INF:
        return INF, None
    # the in-arcs of every node as (source, word, pi, end time); the end node E is node n
    arcs = [[] for _ in range(n + 1)]
    for v in range(n):
        if v == s or fwd[v] == -INF:
            continue
        for j in into[v]:
            u = int(lat.src[j])
            if fwd[u] > -INF and x[j] < INF:
                arcs[v].append((u, word[j], math.exp(fwd[u] - x[j] - fwd[v]), int(lat.time[v])))
    for v, val in stops.items():
        arcs[n].append((v, 0, math.exp(val - log_z), lat.num_frames))
    r = [0]
    for w in hyp:
        r += [0, int(w)]
    r.append(0)                                 # r[1 .. S], S = 2 Q + 1
    S = len(r) - 1

    def sub(w, q):
        return 0.0 if w == r[q] else 1.0 + DELTA

    def ins(w):
        return 0.0 if w == 0 else 1.0 + DELTA

    def dele(q):
        return 0.0 if r[q] == 0 else 1.0

    alpha = [[0.0] * (S + 1) for _ in range(n + 1)]
    for q in range(1, S + 1):
        alpha[s][q] = alpha[s][q - 1] + dele(q)

    def arc_chain(u, w):
        a = [alpha[u][0] + ins(w)]
        for q in range(1, S + 1):
            a.append(min(alpha[u][q - 1] + sub(w, q), alpha[u][q] + ins(w), a[q - 1] + dele(q)))
        return a

    for v in order + [n]:
        if v == s:
            continue
        for u, w, p, _ in arcs[v]:
            a = arc_chain(u, w)
            for q in range(S + 1):
                alpha[v][q] += p * a[q]
    risk = alpha[n][S]
    beta = [[0.0] * (S + 1) for _ in range(n + 1)]
    beta[n][S] = 1.0
    gamma = [dict() for _ in range(S + 1)]

    def add(q, w, m):
        gamma[q][w] = gamma[q].get(w, 0.0) + m

    for v in [n] + order[::-1]:
        if v == s:
            b = 0.0
            for q in range(S, 0, -1):
                b += beta[s][q]
                add(q, 0, b)
            continue
        for u, w, p, _ in arcs[v]:
            a = arc_chain(u, w)
            b = [0.0] * (S + 1)
            for q in range(S, 0, -1):
                b[q] += p * beta[v][q]
                a1 = alpha[u][q - 1] + sub(w, q)
                a2 = alpha[u][q] + ins(w)
                a3 = a[q - 1] + dele(q)
                if a1 <= a2 and a1 <= a3:
                    beta[u][q - 1] += b[q]
                    add(q, w, b[q])
                elif a2 <= a3:
                    beta[u][q] += b[q]
                else:
                    b[q - 1] += b[q]
                    add(q, 0, b[q])
            b[0] += p * beta[v][0]
            beta[u][0] += b[0]
    return risk, gamma
