"""Shared loader of tests/golden/ctc_align.npz (tests/golden/make_golden_align.py): the
reference's forced alignments, loaded once per session and never modified."""
import json

import numpy as np

from conftest import golden

_cache = {}


def data():
    if 'npz' not in _cache:
        z = golden('ctc_align.npz')
        _cache['npz'] = z
        _cache['index'] = json.loads(str(z['index']))
        _cache['mats'] = json.loads(str(z['mats_json']))
    return _cache['npz'], _cache['index'], _cache['mats']


def case(name):
    """dict of one align case: its index entry plus lp, labels, cost, sol, states, segments"""
    key = ('case', name)
    if key not in _cache:
        z, index, _ = data()
        c = dict(next(e for e in index if e['name'] == name))
        for f in ('lp', 'labels', 'cost', 'sol', 'states', 'segments'):
            c[f] = z['%s_%s' % (name, f)]
            c[f].setflags(write=False)
        _cache[key] = c
    return _cache[key]


def names(**where):
    """names of the align cases whose index entries match every given field"""
    return [e['name'] for e in data()[1] if all(e[k] == v for k, v in where.items())]


def group_key(c):
    return (c['kind'], c['S'], c['allow'], c['evalrep'])


def assemble(cases, act_override=None):
    """one batch of cases of the same group: lp [T, B, C] (padding frames zero), flat labels,
    act_lens, label_lens; act_override {b: frames} shortens utterances"""
    assert len({group_key(c) for c in cases}) == 1
    T = max(c['T'] for c in cases)
    C = cases[0]['lp'].shape[1]
    lp = np.zeros((T, len(cases), C), np.float32)
    act = []
    for b, c in enumerate(cases):
        lp[:c['T'], b] = c['lp']
        act.append(c['T'])
    for b, t in (act_override or {}).items():
        act[b] = t
    labels = np.concatenate([c['labels'] for c in cases]).astype(np.int64)
    return lp, labels, act, [c['L'] for c in cases]


def want(cases, T, Lmax, infeasible=()):
    """the golden outputs of a batch in the layout of ctc_viterbi_align_batch"""
    B = len(cases)
    cost = np.full(B, np.inf)
    frames = np.full((B, T), -1, np.int32)
    states = np.full((B, T), -1, np.int32)
    segments = np.full((B, Lmax, 2), -1, np.int32)
    for b, c in enumerate(cases):
        if not c['feasible'] or b in infeasible:
            continue
        cost[b] = c['cost']
        frames[b, :c['T']] = c['sol']
        states[b, :c['T']] = c['states']
        segments[b, :c['L']] = c['segments']
    return cost, frames, states, segments


def flags(c):
    if c['kind'] == 'mono':
        return dict(num_symbols=c['S'], context_order=1)
    return dict(num_symbols=c['S'], context_order=2, allow_nonblank_selfloops=c['allow'],
                eval_repeats_in_context=c['evalrep'])
