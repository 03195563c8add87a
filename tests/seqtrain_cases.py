"""Shared inputs and the brute-force referee of the sequence-training tests (tests/test_lattice_seqtrain.py
on the CPU, tests/test_lattice_seqtrain_gpu.py on the GPU): the lattices of tests/nbest_cases.py with live
scores that differ from the ones frozen at decode time, random frame references, and a referee that
enumerates every complete path of a lattice and differentiates the objective with autograd in fp64."""
import sys

import numpy as np
import torch

import nbest_cases
from nbest_cases import LENS, UNQUANTISED_LENS

from att_speech.wfst_lattice import Lattice, _empty

INF = float('inf')
CRITERIA = ('mmi', 'smbr')
BOOSTS = (0.0, 0.5)
MAX_PATHS = 5000            # the largest lattice enumerated here has 4928 complete paths

_CACHE = {}


def live_scores(decode_scores, seed):
    """the decode scores plus a fixed perturbation, so that s(a) != lp[a]; NaN (frames beyond an
    utterance's length: never to be read) stays NaN.  float32 [T, B, C]"""
    lp = np.asarray(decode_scores, np.float32)
    rng = np.random.default_rng(seed)
    return (lp + rng.uniform(-0.5, 0.5, lp.shape).astype(np.float32)).astype(np.float32)


def random_ref(lats, T, C, seed, from_lattice=False):
    """[B, T] int32: a random class per frame, -1 beyond each utterance's length.  from_lattice: drawn
    among the classes the lattice's arcs read at that frame, so that many arcs are correct even for large C."""
    rng = np.random.default_rng(seed)
    ref = np.full((len(lats), T), -1, np.int32)
    for b, lat in enumerate(lats):
        n = min(int(lat.num_frames), T)
        ref[b, :n] = rng.integers(0, C, n)
        if from_lattice and lat.num_arcs:
            il, k = lat.ilabel, lat.time[lat.dst]
            for t in range(n):
                here = il[(il > 0) & (k == t + 1)]
                if len(here):
                    ref[b, t] = int(rng.choice(here)) - 1
    return ref


def toy_case(name, scale, lb):
    """(lattices, live log_probs [5, 4, 3] float32, ref [4, 5]) of one point of nbest_cases.sweep()"""
    key = ('toy', name, scale, lb)
    if key not in _CACHE:
        lats = nbest_cases.toy_lattices(name, scale, lb)[0]
        lp = live_scores(nbest_cases.toy_inputs(name)[1], 5)
        _CACHE[key] = (lats, lp, random_ref(lats, 5, 3, 7))
    return _CACHE[key]


def unquantised_case(lb):
    """(lattices, live log_probs [24, 4, 49] float32, ref [4, 24]) over the bigram graph"""
    key = ('unq', lb)
    if key not in _CACHE:
        lats = nbest_cases.unquantised_lattices(lb)
        lp = live_scores(nbest_cases.unquantised_scores().numpy(), 9)
        _CACHE[key] = (lats, lp, random_ref(lats, 24, 49, 13, from_lattice=True))
    return _CACHE[key]


def fan_case():
    """(lattices, live log_probs [3, 1, 3] float32, ref [1, 3]) of the hand-made fan lattice"""
    if 'fan' not in _CACHE:
        lat = nbest_cases.fan_lattice(3000)
        lp = np.random.default_rng(17).uniform(-3.0, 0.0, (3, 1, 3)).astype(np.float32)
        _CACHE['fan'] = ([lat], lp, random_ref([lat], 3, 3, 19))
    return _CACHE['fan']


def mixed_case():
    """(lattices, live log_probs, ref): toy a's lattices with an empty lattice in the middle and one
    utterance that did not reach a final state (every node of its last frame ends a path at cost 0)"""
    if 'mixed' not in _CACHE:
        lats, lp, ref = toy_case('a', 1.0, 2.0)
        lats = list(lats)
        g = lats[0].graph
        lats[1] = _empty(g, 1.0, LENS[1])
        l = lats[2]
        lats[2] = Lattice(g, l.acoustic_scale, l.num_frames, l.cost, False, *[getattr(l, f) for f in Lattice.FIELDS])
        _CACHE['mixed'] = (lats, lp, ref)
    return _CACHE['mixed']


def complete_paths(lat, lm_scale=1.0):
    """every complete path of a lattice by depth-first search: (list of arc index lists, end node per
    path); the start node is the first (time 0, start state) node, an end node has a finite end cost"""
    n = lat.num_nodes
    if not n:
        return [], []
    starts = np.nonzero((lat.time == 0) & (lat.state == lat.graph.start))[0]
    if not len(starts):
        return [], []
    end = lat._end_costs(lm_scale)
    out_ptr = np.searchsorted(lat.src, np.arange(n + 1))
    paths, ends, stack = [], [], []
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))

    def walk(v):
        if end[v] < INF:
            assert len(paths) < MAX_PATHS, "too many paths to enumerate"
            paths.append(list(stack))
            ends.append(v)
        for a in range(out_ptr[v], out_ptr[v + 1]):
            stack.append(a)
            walk(int(lat.dst[a]))
            stack.pop()
    walk(int(starts[0]))
    return paths, ends


def brute_force(lats, log_probs, ref, criterion, acoustic_scale, lm_scale, boost):
    """objective [B] and d objective[b] / d log_probs [T, B, C] by enumeration: torch fp64, the path costs
    as sums of lm w - sc s + boost acc plus lm end, logsumexp ('mmi') or the probability-weighted path
    accuracy ('smbr'), differentiated by autograd.  Also the number of complete paths per utterance."""
    lp = torch.tensor(np.asarray(log_probs, np.float64), requires_grad=True)
    T, B, C = lp.shape
    objective = np.full(B, 0.0 if criterion == 'smbr' else -INF)
    counts, total = [], None
    for b, lat in enumerate(lats):
        paths, ends = complete_paths(lat, lm_scale)
        counts.append(len(paths))
        if not paths:
            continue
        sc = lat.acoustic_scale if acoustic_scale is None else float(acoustic_scale)
        il = torch.from_numpy(lat.ilabel.astype(np.int64))
        k = torch.from_numpy(lat.time[lat.dst].astype(np.int64))
        em = il > 0
        s = torch.zeros(lat.num_arcs, dtype=torch.float64)
        s = s.masked_scatter(em, lp[k[em] - 1, b, il[em] - 1])
        acc = torch.zeros(lat.num_arcs, dtype=torch.float64)
        if ref is not None:
            r = torch.from_numpy(np.asarray(ref, np.int64))[b]
            acc[em] = (r[k[em] - 1] == il[em] - 1).double()
        x = float(lm_scale) * torch.from_numpy(lat.w.astype(np.float64)) - sc * s + float(boost) * acc
        pid = torch.tensor([i for i, p in enumerate(paths) for _ in p], dtype=torch.int64)
        aid = torch.tensor([a for p in paths for a in p], dtype=torch.int64)
        cost = torch.from_numpy(lat._end_costs(lm_scale)[ends]).clone()
        cost = cost.index_add(0, pid, x[aid])
        pacc = torch.zeros(len(paths), dtype=torch.float64).index_add(0, pid, acc[aid])
        if not bool((cost < INF).any()):
            continue
        if criterion == 'mmi':
            value = torch.logsumexp(-cost, 0)
        else:
            value = (torch.softmax(-cost, 0) * pacc).sum()
        objective[b] = float(value.detach())
        total = value if total is None else total + value
    grad = np.zeros((T, B, C))
    if total is not None and total.requires_grad:
        total.backward()
        grad = np.nan_to_num(lp.grad.numpy(), nan=0.0)
    return objective, grad, counts


def arc_sums(batch_arrays, arc_grad, T, B, C):
    """arc_grad summed per (frame, class) in fp64 in ascending arc order, [T, B, C] float64, from
    (ilabel [A], time of the destination [A], utterance [A])"""
    il, k, utt = [np.asarray(v, np.int64) for v in batch_arrays]
    em = il > 0
    out = np.zeros(T * B * C)
    np.add.at(out, ((k[em] - 1) * B + utt[em]) * C + il[em] - 1, np.asarray(arc_grad, np.float64)[em])
    return out.reshape(T, B, C)


def host_arrays(hb):
    """(ilabel, destination time, utterance) per arc of a LatticeBatch"""
    return hb.graph.ilabel[hb.arc], hb.time[hb.dst], hb.n_utt[hb.src]
