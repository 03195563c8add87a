#!/usr/bin/env python
"""tests/golden/make_golden_align.py — regenerates tests/golden/ctc_align.npz.

Runs ONLY where the reference checkout exists (/root/reference): it imports the reference's own
att_speech.modules.ctc_losses under the installed Python, with empty stub modules for the absent
third-party packages, and records what its alignment and decoding functions return.  Data only;
nothing of the reference's source travels.

One shim: under the installed torch and numpy, raw_generic_viterbi's
`assert np.all(B.sum(0) == 1)` raises a TypeError, because a tensor is handed to np.all.  The
reference module's `np` attribute is therefore set to a thin proxy whose `all` converts its
argument with np.asarray first and which forwards every other attribute to numpy.  The
reference's arithmetic is untouched.

Every case stores float32 log-probs (log_softmax of seeded normals; `q`: rounded to multiples of
0.5, `k`: whole frames constant, both to force exact ties), the labels, and the reference's
(cost, sol).  Align cases also store the reference's STATE path: raw_generic_viterbi run again on
the gathered emissions lp.dot(B) with an identity emission matrix, so that its `sol` is the state
index, and the label segments read off that path.  For an infeasible case (cost = inf) only the
cost is meaningful: the reference walks back-pointers of unreachable states there.

  index        JSON list of the cases: name, kind, S, flags, T, L, feasible
  <name>_lp / _labels / _cost / _sol / _states / _segments
  mats_json    label sequences and options of the recorded dense builder outputs mats_<k>_A / _B

Usage:  python tests/golden/make_golden_align.py
"""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'

for name in ['pywrapfst', 'torchtext', 'torchtext.vocab', 'kaldi_io', 'tensorboardX']:
    sys.modules[name] = types.ModuleType(name)
sys.modules['torchtext'].vocab = sys.modules['torchtext.vocab']
sys.modules['torchtext.vocab'].Vocab = object
sys.modules['tensorboardX'].SummaryWriter = object
sys.path.insert(0, REF)

import numpy as np          # noqa: E402
import torch                # noqa: E402

warnings.filterwarnings('ignore')

from att_speech.modules import ctc_losses as ref      # noqa: E402  (the REFERENCE's module)


class _NumpyProxy(object):
    """numpy, except that `all` accepts a tensor"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def all(x, *args, **kwargs):
        return np.all(np.asarray(x), *args, **kwargs)


ref.np = _NumpyProxy()

FLAGS = [(a, e) for a in (True, False) for e in (False, True)]   # (allow_nonblank_selfloops, eval_repeats_in_context)


def log_probs(rng, T, C, mode):
    x = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32)), -1).numpy()
    if mode == 'q':
        x = np.round(x * 2) / 2
    elif mode == 'k':
        x = np.round(x * 2) / 2
        x[::2] = x[0, 0]                    # every other frame constant over the classes
        if T > 2:
            x[1] = -1.5
    return np.ascontiguousarray(x, np.float32)


def transcript(rng, L, S, repeats):
    while True:
        lab = rng.randint(1, S, size=L)
        has = L > 1 and bool((lab[1:] == lab[:-1]).any())
        if L == 1 or S == 2 or has == repeats:
            return lab.astype(np.int64)
        if repeats:
            k = rng.randint(0, L - 1)
            lab[k + 1] = lab[k]
            if L > 2 and rng.randint(2):    # a triple: the case eval_repeats_in_context is about
                k = min(k, L - 3)
                lab[k + 1] = lab[k + 2] = lab[k]
            return lab.astype(np.int64)


def segments_of(states, L):
    seg = np.full((L, 2), -1, np.int32)
    first = np.nonzero(np.r_[True, states[1:] != states[:-1]])[0]
    last = np.r_[first[1:], len(states)]
    for f, l in zip(first, last):
        if states[f] % 2 == 1:
            seg[states[f] // 2] = (f, l)
    return seg


def align_case(out, index, name, kind, lp, lab, S, allow=True, evalrep=False):
    lpt, labt = torch.from_numpy(lp), torch.from_numpy(lab)
    if kind == 'mono':
        A, B = ref.get_CTC_matrices_mono(labt, S)
        cost, sol = ref.mono_CTC_viterbi_align(lpt, labt)
    else:
        kw = dict(allow_nonblank_selfloops=allow, eval_repeats_in_context=evalrep)
        A, B = ref.get_CTC_matrices_bicontext(labt, S, **kw)
        cost, sol = ref.bi_CTC_viterbi_align(lpt, labt, **kw)
    N = A.size(0)
    gathered = torch.from_numpy(lp.dot(B.numpy()))
    cost2, states = ref.raw_generic_viterbi(gathered, A, torch.eye(N), start_states=[0, 1],
                                            terminal_states=[N - 2, N - 1])
    assert cost2 == cost or (np.isinf(cost2) and np.isinf(cost))
    states = states.numpy().astype(np.int32)
    feasible = bool(np.isfinite(cost))
    if feasible:
        assert (B.numpy().argmax(0)[states] == sol.numpy()).all()
    out[name + '_lp'] = lp
    out[name + '_labels'] = lab.astype(np.int32)
    out[name + '_cost'] = np.float64(cost)
    out[name + '_sol'] = sol.numpy().astype(np.int32)
    out[name + '_states'] = states
    out[name + '_segments'] = segments_of(states, len(lab))
    index.append(dict(name=name, kind=kind, S=S, allow=allow, evalrep=evalrep, T=int(lp.shape[0]),
                      L=int(len(lab)), feasible=feasible))


def main():
    rng = np.random.RandomState(415)
    out, index = {}, []
    modes = ['n', 'q', 'k']
    n = 0
    # mono, S = 7
    for L in range(1, 7):
        for T in sorted({1, 2, L, 2 * L + 1, 30}):
            for rep in (False, True):
                mode = modes[n % 3]
                n += 1
                align_case(out, index, 'mono_L%d_T%d_%s%s' % (L, T, 'r' if rep else 'u', mode), 'mono',
                           log_probs(rng, T, 7, mode), transcript(rng, L, 7, rep), 7)
    # bicontext, S = 5 and 7, all four flag settings
    for S, Ls in ((5, (1, 2, 3, 4, 5, 6)), (7, (2, 5))):
        for allow, ev in FLAGS:
            for L in Ls:
                Ts = {L, 2 * L + 1} | ({1, 2, 30} if L in (1, 3, 5) else set())
                for T in sorted(Ts):
                    for rep in ((False, True) if T >= L else (False,)):
                        mode = modes[n % 3]
                        n += 1
                        name = 'bi%d_%d%d_L%d_T%d_%s%s' % (S, allow, ev, L, T, 'r' if rep else 'u', mode)
                        align_case(out, index, name, 'bi', log_probs(rng, T, S * S, mode),
                                   transcript(rng, L, S, rep), S, allow, ev)
    # a triple repeat under every flag setting, quantised
    for allow, ev in FLAGS:
        align_case(out, index, 'bi5_%d%d_triple' % (allow, ev), 'bi', log_probs(rng, 12, 25, 'q'),
                   np.array([2, 2, 2, 3, 3], np.int64), 5, allow, ev)
    align_case(out, index, 'bi49_L4_T12', 'bi', log_probs(rng, 12, 49 * 49, 'n'),
               np.array([7, 48, 48, 1], np.int64), 49)
    # kernel-boundary shapes, C = 7
    for L in (31, 32, 33, 127, 128, 129):
        align_case(out, index, 'edge_mono_L%d' % L, 'mono', log_probs(rng, 2 * L, 7, 'q' if L % 2 else 'n'),
                   transcript(rng, L, 7, True), 7)
    align_case(out, index, 'edge_mono_L511_T1100', 'mono', log_probs(rng, 1100, 7, 'n'),
               transcript(rng, 511, 7, True), 7)
    # N = 255 has 64 bytes of back-pointers per frame: 768 frames are 48 KiB, 769 are more
    align_case(out, index, 'edge_mono_L127_T768', 'mono', log_probs(rng, 768, 7, 'q'),
               transcript(rng, 127, 7, True), 7)
    align_case(out, index, 'edge_mono_L127_T769', 'mono', log_probs(rng, 769, 7, 'q'),
               transcript(rng, 127, 7, True), 7)
    for i, (allow, ev) in enumerate(FLAGS):      # bicontext across a wave boundary, S = 2: C = 4
        align_case(out, index, 'edge_bi2_%d%d_L%d' % (allow, ev, 33 + i), 'bi',
                   log_probs(rng, 150, 4, 'q'), np.ones(33 + i, np.int64), 2, allow, ev)

    # frame-level decoding, S = 5
    lp = log_probs(rng, 12, 5, 'q')
    cost, sol = ref.mono_CTC_viterbi_decode(torch.from_numpy(lp))
    out.update(dec_mono_lp=lp, dec_mono_cost=np.float64(cost), dec_mono_sol=sol.numpy())
    for ev in (False, True):
        lp = log_probs(rng, 12, 25, 'q' if ev else 'n')
        cost, sol = ref.bi_CTC_viterbi_decode(torch.from_numpy(lp), eval_repeats_in_context=ev)
        out.update({'dec_bi%d_lp' % ev: lp, 'dec_bi%d_cost' % ev: np.float64(cost),
                    'dec_bi%d_sol' % ev: sol.numpy()})
    # raw_generic_viterbi without start / terminal states, on a mono lattice
    lp, lab = log_probs(rng, 9, 7, 'q'), np.array([3, 3, 1], np.int64)
    A, B = ref.get_CTC_matrices_mono(torch.from_numpy(lab), 7)
    cost, sol = ref.raw_generic_viterbi(torch.from_numpy(lp), A, B)
    out.update(raw_lp=lp, raw_labels=lab, raw_cost=np.float64(cost), raw_sol=sol.numpy())
    # loop_using_symbol_repetitions: the 3 L + 1 lattice
    lp, lab = log_probs(rng, 14, 25, 'n'), np.array([1, 1, 4, 2], np.int64)
    cost, sol = ref.bi_CTC_viterbi_align(torch.from_numpy(lp), torch.from_numpy(lab),
                                         loop_using_symbol_repetitions=True)
    out.update(loop_lp=lp, loop_labels=lab, loop_cost=np.float64(cost), loop_sol=sol.numpy())

    # dense builder outputs
    mats = []

    def record(what, A, B, **kw):
        k = len(mats)
        out['mats_%d_A' % k], out['mats_%d_B' % k] = A.numpy().astype(np.int8), B.numpy().astype(np.int8)
        mats.append(dict(what=what, **kw))
    lab = [1, 3, 3, 3, 2, 2, 4]
    record('mono', *ref.get_CTC_matrices_mono(torch.tensor(lab), 5), labels=lab, S=5)
    for allow, ev in FLAGS:
        record('bi', *ref.get_CTC_matrices_bicontext(torch.tensor(lab), 5, eval_repeats_in_context=ev,
                                                     allow_nonblank_selfloops=allow),
               labels=lab, S=5, allow=allow, evalrep=ev)
    record('bi_loop', *ref.get_CTC_matrices_bicontext(torch.tensor(lab), 5, loop_using_symbol_repetitions=True),
           labels=lab, S=5)
    record('bi_looprepeats', *ref.get_CTC_matrices_bicontext_looprepeats(torch.tensor(lab), 5), labels=lab, S=5)
    record('dec_mono', *ref.get_CTC_decoding_matrices_mono(5), S=5)
    for ev in (False, True):
        record('dec_bi', *ref.get_CTC_decoding_matrices_bicontext(4, eval_repeats_in_context=ev), S=4, evalrep=ev)

    out['index'] = np.array(json.dumps(index))
    out['mats_json'] = np.array(json.dumps(mats))
    path = os.path.join(HERE, 'ctc_align.npz')
    np.savez_compressed(path, **out)
    print('%s: %d align cases (%d infeasible), %d bytes' % (
        path, len(index), sum(not c['feasible'] for c in index), os.path.getsize(path)))


if __name__ == '__main__':
    main()
