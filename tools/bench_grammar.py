#!/usr/bin/env python
"""Denominator forward-backward and Viterbi over HC o G decoding graphs (mono CTC composed with
the reference's character bigram / trigram LM, tests/golden/G_char_*_syms.fst.gz) at the
benchmark's frame count: the shared-graph kernel (csrc/lattice_shared.hip) against the generic
lattice kernel on the padded matrices of the same graph (ASR_SHARED_NATIVE=0).

    python tools/bench_grammar.py [--batch 768] [--frames 334] [--reps 5] [--lms bigram,trigram]

Prints one JSON line per (graph, kernel): median, min and max of `reps` timed calls after two
warm-up calls, each call timed with device events around it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-asr_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(out)), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=768)
    ap.add_argument('--frames', type=int, default=334)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lms', default='bigram,trigram')
    ap.add_argument('--kernels', default='shared,generic')
    a = ap.parse_args()
    from att_speech import _native, fst_utils as P
    dev = torch.device('cuda:0')
    golden = os.path.join(ROOT, 'tests', 'golden')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    x = torch.from_numpy(rng.standard_normal((T, B, 49)).astype(np.float32) * 2).to(dev)
    lp = x - x.max(-1, keepdim=True)[0]
    lens = torch.from_numpy(np.sort(rng.integers(T // 2, T + 1, size=B))[::-1].astype(np.int32).copy()).to(dev)
    for name in a.lms.split(','):
        gg = P.CTCGraphGen(context_order=1, num_symbols=49,
                           grammar_fst=os.path.join(golden, 'G_char_%s_syms.fst.gz' % {'bigram': 'bg', 'trigram': 'tg'}[name]),
                           vocabulary=os.path.join(golden, 'wsj_vocabulary.txt'))
        tagged = gg.get_decoding_matrices()
        sg = _native.SharedGraph(tagged.shared, dev)
        runs = {}
        if 'shared' in a.kernels:
            runs['shared'] = (lambda: _native.shared_fwbw(lp, lens, sg, -1e20),
                              lambda: _native.shared_forward(lp, lens, sg, -1e20, viterbi=True, want_path=True))
        if 'generic' in a.kernels:
            g = _native.Graph(list(tagged), dev)
            runs['generic'] = (lambda: _native.lattice_fwbw(lp, lens, g, -1e20),
                               lambda: _native.lattice_forward(lp, lens, g, -1e20, viterbi=True, want_path=True))
        for kern, (fwbw, vit) in runs.items():
            print(json.dumps(dict(graph='mono_' + name, kernel=kern, states=sg.N, arcs=sg.E, frames=T, batch=B,
                                  fwbw=timed(fwbw, a.reps), viterbi=timed(vit, a.reps))), flush=True)


if __name__ == '__main__':
    main()
