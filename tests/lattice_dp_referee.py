"""Referee of the lattice dynamic programmes (att_speech.lattice_dp, LatticeBatch.posteriors): every
complete path of a small lattice is enumerated by depth-first search over the arc arrays, scored in
fp64 one path at a time, and the posteriors are direct sums over those paths.  Shares no code with
the implementation: no levels, no dynamic programme."""
import math

INF = float('inf')


def _end_cost(lat, v):
    """the unscaled cost of stopping at node v, None when v is no end node"""
    if int(lat.time[v]) != lat.num_frames:
        return None
    if not lat.reached_final:
        return 0.0
    f = float(lat.graph.final[int(lat.state[v])])
    return f if f < INF else None


def _scales(lat, acoustic_scale, lm_scale):
    return (lat.acoustic_scale if acoustic_scale is None else float(acoustic_scale)), float(lm_scale)


def _arc_cost(lat, j, sc, lm):
    g = int(lat.arc[j])
    return lm * float(lat.graph.weight[g]) - sc * float(lat.lp[j])


def complete_paths(lat, max_paths=200000):
    """[(arc positions in path order, end node)] of every path from the start node to an end node"""
    out_arcs = [[] for _ in range(lat.num_nodes)]
    for j in range(lat.num_arcs):
        out_arcs[int(lat.src[j])].append(j)
    starts = [v for v in range(lat.num_nodes) if lat.time[v] == 0 and lat.state[v] == lat.graph.start]
    paths = []
    if not starts:
        return paths
    stack = [(starts[0], [])]
    while stack:
        v, arcs = stack.pop()
        if _end_cost(lat, v) is not None:
            paths.append((arcs, v))
            assert len(paths) <= max_paths, "lattice too large for the enumerator"
        for j in out_arcs[v]:
            stack.append((int(lat.dst[j]), arcs + [j]))
    return paths


def scored_paths(lat, acoustic_scale=None, lm_scale=1.0):
    """per complete path a dict: arcs, end, cost (scaled, with the end cost), graph_cost,
    acoustic_cost (unscaled) and words"""
    sc, lm = _scales(lat, acoustic_scale, lm_scale)
    out = []
    for arcs, v in complete_paths(lat):
        cost = 0.0
        for j in arcs:
            cost = cost + _arc_cost(lat, j, sc, lm)
        end = _end_cost(lat, v)
        g = [int(lat.arc[j]) for j in arcs]
        out.append(dict(arcs=arcs, end=v, cost=cost + lm * end,
                        graph_cost=end + sum(float(lat.graph.weight[a]) for a in g),
                        acoustic_cost=-sum(float(lat.lp[j]) for j in arcs),
                        words=[int(lat.graph.olabel[a]) for a in g if lat.graph.olabel[a] != 0]))
    return out


def _log_sum(values):
    values = [v for v in values if v > -INF]
    if not values:
        return -INF
    m = max(values)
    return m + math.log(math.fsum(math.exp(v - m) for v in values))


def posteriors(lat, acoustic_scale=None, lm_scale=1.0):
    """(log_z, [log posterior per arc], [log posterior per node]) by direct summation over the paths"""
    paths = scored_paths(lat, acoustic_scale, lm_scale)
    log_z = _log_sum([-p['cost'] for p in paths])
    by_arc = [[] for _ in range(lat.num_arcs)]
    by_node = [[] for _ in range(lat.num_nodes)]
    for p in paths:
        nodes = {p['end']}
        for j in p['arcs']:
            by_arc[j].append(-p['cost'])
            nodes.add(int(lat.src[j]))
        for v in nodes:
            by_node[v].append(-p['cost'])

    def rel(group):
        s = _log_sum(group)
        return s - log_z if s > -INF else -INF
    return log_z, [rel(g) for g in by_arc], [rel(g) for g in by_node]


def best_path(lat, acoustic_scale=None, lm_scale=1.0):
    """(words, cost, graph_cost, acoustic_cost) under the tie rule of Lattice.best_path: a node's cost
    is the cheapest prefix into it; its back-pointer the in-arc of the smallest GRAPH arc index among
    those that attain that cost; the end node the smallest index among the cheapest totals."""
    none = ([], INF, INF, INF)
    if not lat.num_nodes:
        return none
    sc, lm = _scales(lat, acoustic_scale, lm_scale)
    out_arcs = [[] for _ in range(lat.num_nodes)]
    for j in range(lat.num_arcs):
        out_arcs[int(lat.src[j])].append(j)
    starts = [v for v in range(lat.num_nodes) if lat.time[v] == 0 and lat.state[v] == lat.graph.start]
    if not starts:
        return none
    cost = [INF] * lat.num_nodes
    stack = [(starts[0], 0.0)]
    while stack:                                # every prefix, summed from the start
        v, c = stack.pop()
        cost[v] = min(cost[v], c)
        for j in out_arcs[v]:
            stack.append((int(lat.dst[j]), c + _arc_cost(lat, j, sc, lm)))
    ends = [(cost[v] + lm * _end_cost(lat, v), v) for v in range(lat.num_nodes)
            if _end_cost(lat, v) is not None and cost[v] < INF]
    if not ends:
        return none
    total, v = min(ends)
    end = _end_cost(lat, v)
    gc, ac, words = end, 0.0, []
    while v != starts[0]:
        into = [j for j in range(lat.num_arcs) if int(lat.dst[j]) == v
                and cost[int(lat.src[j])] + _arc_cost(lat, j, sc, lm) == cost[v]]
        j = min(into, key=lambda k: int(lat.arc[k]))
        g = int(lat.arc[j])
        gc += float(lat.graph.weight[g])
        ac -= float(lat.lp[j])
        if lat.graph.olabel[g] != 0:
            words.append(int(lat.graph.olabel[g]))
        v = int(lat.src[j])
    return words[::-1], total, gc, ac
