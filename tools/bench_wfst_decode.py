#!/usr/bin/env python
"""Beam-pruned WFST decoding (att_speech.wfst_decode.decode_graph, csrc/wfst_decode.hip) at the
benchmark's frame count: T' = 334, lengths uniform in [167, 334].

    python tools/bench_wfst_decode.py [--batch 768] [--frames 334] [--reps 5] [--lms bigram,trigram]
        [--beams inf,16,8] [--synthetic-states 1000000] [--synthetic-batch 16] [--synthetic-beams 8,16,20]
        [--sweep-threads 256,512,1024] [--out FILE.json]

mono o bigram / mono o trigram (tests/golden/G_char_*_syms.fst.gz through CTCGraphGen): the pruned
search at each beam against the exact every-state Viterbi of the same call (csrc/lattice_shared.hip).
A synthetic graph of about `--synthetic-states` states and three arcs a state: the device against
the host path.  Prints one JSON line per measurement: median, min and max of `reps` calls after two
warm-up calls, each timed with device events around it (the host path with the wall clock, once),
and the mean number of active tokens per frame so the time can be read against the work.
--sweep-threads then repeats a shorter table (beams inf and 8, synthetic beam 16, 3 calls) with the
given threads per workgroup instead of the kernel's own choice; --out holds both (`rows`,
`threads_ab`)."""
import argparse
import json
import os
import sys
import time

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


def mean_active(res, lens):
    na = res['num_active'].cpu().numpy()
    mask = np.arange(na.shape[1])[None, :] < np.asarray(lens)[:, None]
    return float(na[mask].mean())


def synthetic_graph(rng, N, C, arcs_per_state=3, n_words=20000):
    """random sparse graph: a tenth of the arcs are epsilon arcs that lead to a higher state id
    (acyclic), a tenth of the states are final"""
    from att_speech.wfst_decode import DecodingGraph
    A = N * arcs_per_state
    src = rng.integers(0, N, size=A)
    dst = rng.integers(0, N, size=A)
    il = rng.integers(1, C + 1, size=A)
    eps = (rng.random(A) < 0.1) & (dst > src) & (src % 2 == 0) & (dst % 2 == 1)
    il[eps] = 0
    ol = np.where(rng.random(A) < 0.2, rng.integers(1, n_words + 1, size=A), 0)
    w = (rng.random(A) * 6).astype(np.float32)
    final = np.where(rng.random(N) < 0.1, rng.random(N), np.inf)
    return DecodingGraph(N, 0, src, dst, il, ol, w, final)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=768)
    ap.add_argument('--frames', type=int, default=334)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lms', default='bigram,trigram')
    ap.add_argument('--beams', default='inf,16,8')
    ap.add_argument('--synthetic-states', type=int, default=1000000)
    ap.add_argument('--synthetic-batch', type=int, default=16)
    ap.add_argument('--synthetic-beams', default='8,16,20')
    ap.add_argument('--synthetic-classes', type=int, default=200)
    ap.add_argument('--workspace-mb', type=int, default=8192)
    ap.add_argument('--sweep-threads', default='',
                    help='A/B: comma list of 256, 512, 1024 threads per workgroup, measured after the main table')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from att_speech import _native, fst_utils as P, wfst_decode
    from att_speech.wfst_decode import DecodingGraph, decode_graph, decode_graph_host
    dev = torch.device('cuda:0')
    golden = os.path.join(ROOT, 'tests', 'golden')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    ws = a.workspace_mb << 20
    rows, threads_ab = [], []
    sink = rows

    def emit(row):
        if wfst_decode.THREADS_PER_WORKGROUP:
            row['threads'] = wfst_decode.THREADS_PER_WORKGROUP
        sink.append(row)
        print(json.dumps(row), flush=True)

    x = torch.from_numpy(rng.standard_normal((T, B, 49)).astype(np.float32) * 2).to(dev)
    lp = x - x.max(-1, keepdim=True)[0]
    lens_np = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    lens = torch.from_numpy(lens_np).to(dev)
    lm_graphs = {}
    for name in [n for n in a.lms.split(',') if n]:
        gg = P.CTCGraphGen(context_order=1, num_symbols=49,
                           grammar_fst=os.path.join(golden, 'G_char_%s_syms.fst.gz' % {'bigram': 'bg', 'trigram': 'tg'}[name]),
                           vocabulary=os.path.join(golden, 'wsj_vocabulary.txt'))
        lm_graphs[name] = (_native.SharedGraph(gg.get_decoding_matrices().shared, dev),
                           DecodingGraph.from_graph_generator(gg))
    if a.synthetic_states > 0:
        N, Bs, C = a.synthetic_states, a.synthetic_batch, a.synthetic_classes
        g = synthetic_graph(rng, N, C)
        xs = torch.from_numpy(rng.standard_normal((T, Bs, C)).astype(np.float32) * 3)
        lps = torch.log_softmax(xs, -1)
        ls = rng.integers(T // 2, T + 1, size=Bs).astype(np.int32)
        lpd = lps.to(dev)

    def measure(beams, syn_beams, reps):
        for name in [n for n in a.lms.split(',') if n]:
            sg, dg = lm_graphs[name]
            exact = timed(lambda: _native.shared_forward(lp, lens, sg, -1e20, viterbi=True, want_path=True), reps)
            emit(dict(graph='mono_' + name, search='exact_viterbi', states=sg.N, arcs=sg.E, frames=T, batch=B, **exact))
            score = _native.shared_forward(lp, lens, sg, -1e20, viterbi=True, want_path=True)[0].cpu().numpy()
            for beam in [float(b) for b in beams.split(',')]:
                res = decode_graph(lp, lens_np, dg, beam=beam, workspace_bytes=ws)
                t = timed(lambda: decode_graph(lp, lens_np, dg, beam=beam, workspace_bytes=ws), reps)
                cost = res['cost'].cpu().numpy()
                emit(dict(graph='mono_' + name, search='beam', beam=beam, states=dg.num_states, arcs=len(dg.src),
                          frames=T, batch=B, mean_active=mean_active(res, lens_np),
                          redone_on_host=len(res['redone_on_host']),
                          same_score_as_exact=float(np.mean(np.abs(cost + score) <= 1e-3 * np.abs(score))),
                          vs_exact=t['median_ms'] / exact['median_ms'], **t))
        if a.synthetic_states > 0:
            for beam in [float(b) for b in syn_beams.split(',')]:
                res = decode_graph(lpd, ls, g, beam=beam, workspace_bytes=ws)
                t = timed(lambda: decode_graph(lpd, ls, g, beam=beam, workspace_bytes=ws), reps)
                t0 = time.perf_counter()
                host = decode_graph_host(lps.numpy(), ls, g, beam=beam)
                host_ms = (time.perf_counter() - t0) * 1e3
                same = bool((res['cost'].cpu().numpy().view(np.int32) == host['cost'].view(np.int32)).all()
                            and res['words'] == host['words'])
                emit(dict(graph='synthetic', search='beam', beam=beam, states=N, arcs=len(g.src),
                          eps_ranks=g.num_ranks, classes=C, frames=T, batch=Bs, mean_active=mean_active(res, ls),
                          redone_on_host=len(res['redone_on_host']), host_ms=host_ms, same_bits_as_host=same,
                          host_over_device=host_ms / t['median_ms'], **t))
    measure(a.beams, a.synthetic_beams, a.reps)
    sink = threads_ab
    for nt in [int(v) for v in a.sweep_threads.split(',') if v]:
        wfst_decode.THREADS_PER_WORKGROUP = nt
        measure('inf,8', '16', 3)
    wfst_decode.THREADS_PER_WORKGROUP = 0
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_wfst_decode.py', reps=a.reps, rows=rows, threads_ab=threads_ab),
                      f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
