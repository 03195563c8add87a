#!/usr/bin/env python
"""n-best lists from lattices that stay on the device (DeviceLatticeBatch.nbest, asr_lattice_nbest_f64
of csrc/lattice_dp.hip) on the inputs of tools/bench_lattice_dp.py: T' = 334, lengths uniform in
[167, 334]; mono o bigram / mono o trigram at 768 utterances, a synthetic graph of about
`--synthetic-states` states at 16.

    python tools/bench_nbest.py [--batch 768] [--frames 334] [--reps 5] [--lms bigram,trigram] [--beam 16]
        [--lattice-beams 2,8] [--ns 10,64] [--threads 64,256] [--synthetic-states 1000000]
        [--synthetic-batch 16] [--host-utterances 32] [--pkg DIR --baseline-only] [--baseline-json FILE]
        [--out FILE.json]

One JSON line per (graph, lattice beam, n): medians of `reps` calls after two warm-up calls, device
events around the whole call.
  nbest_ms[threads]    the whole batch.nbest(n) call: launch, read-back, the Python lists
  launch_ms[threads]   the launch alone (DeviceLatticeBatch._nbest_launch and a synchronise)
--baseline-only: the path this replaces, batch.lattices() + Lattice.nbest(n) per utterance, timed with
the host clock.  It uses nothing this tool's commit added, so `--pkg DIR` can point it at the package
of a checkout of the parent commit (the same seed draws the same inputs).  lattices_ms is the copy of
the whole batch; Lattice.nbest is timed on the first `--host-utterances` utterances and
host_nbest_ms_scaled is that time scaled to the batch (as profiles/r13_rescore.json did); the sum is
host_ms_scaled.  --baseline-json: such a run's --out file; its rows are joined to this run's and
speedup = host_ms_scaled / the best nbest_ms."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=768)
    ap.add_argument('--frames', type=int, default=334)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lms', default='bigram,trigram')
    ap.add_argument('--beam', type=float, default=16.0)
    ap.add_argument('--lattice-beams', default='2,8')
    ap.add_argument('--ns', default='10,64')
    ap.add_argument('--threads', default='64,256', help='lanes per workgroup to time, the first listed first')
    ap.add_argument('--synthetic-states', type=int, default=1000000)
    ap.add_argument('--synthetic-batch', type=int, default=16)
    ap.add_argument('--synthetic-beam', type=float, default=16.0)
    ap.add_argument('--synthetic-classes', type=int, default=200)
    ap.add_argument('--workspace-mb', type=int, default=32768)
    ap.add_argument('--host-utterances', type=int, default=32)
    ap.add_argument('--pkg', default=os.path.join(ROOT, 'pytorch-asr_amd'), help='the directory that holds att_speech')
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--baseline-json', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    for p in (a.pkg, os.path.join(ROOT, 'tools')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from att_speech import fst_utils as P, lattice_dp, wfst_lattice         # from --pkg: before the tools' own path
    from att_speech.lattice_dp import decode_lattice_device
    from att_speech.wfst_decode import DecodingGraph
    from bench_wfst_decode import synthetic_graph, timed
    assert os.path.realpath(lattice_dp.__file__).startswith(os.path.realpath(a.pkg)), lattice_dp.__file__
    parent = os.path.realpath(a.pkg) != os.path.realpath(os.path.join(ROOT, 'pytorch-asr_amd'))
    dev = torch.device('cuda:0')
    golden = os.path.join(ROOT, 'tests', 'golden')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    ws = a.workspace_mb << 20
    ns = [int(v) for v in a.ns.split(',')]
    threads = [int(v) for v in a.threads.split(',')]
    baseline = {}
    if a.baseline_json:
        for r in json.load(open(a.baseline_json))['rows']:
            baseline[(r['graph'], float(r['lattice_beam']), int(r['n']))] = r
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:                                       # after every row: a run cut short keeps what it measured
            with open(a.out, 'w') as f:
                json.dump(dict(tool='tools/bench_nbest.py', reps=a.reps, baseline_only=a.baseline_only, rows=rows), f,
                          indent=1)
                f.write('\n')

    # the draws of tools/bench_wfst_decode.py, in its order
    x = torch.from_numpy(rng.standard_normal((T, B, 49)).astype(np.float32) * 2).to(dev)
    lp = x - x.max(-1, keepdim=True)[0]
    lens_np = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    cases = []
    for name in [n for n in a.lms.split(',') if n]:
        gg = P.CTCGraphGen(context_order=1, num_symbols=49,
                           grammar_fst=os.path.join(golden, 'G_char_%s_syms.fst.gz' % {'bigram': 'bg', 'trigram': 'tg'}[name]),
                           vocabulary=os.path.join(golden, 'wsj_vocabulary.txt'))
        cases.append(('mono_' + name, DecodingGraph.from_graph_generator(gg), lp, lens_np, a.beam))
    if a.synthetic_states > 0:
        g = synthetic_graph(rng, a.synthetic_states, a.synthetic_classes)
        xs = torch.from_numpy(rng.standard_normal((T, a.synthetic_batch, a.synthetic_classes)).astype(np.float32) * 3)
        ls = rng.integers(T // 2, T + 1, size=a.synthetic_batch).astype(np.int32)
        cases.append(('synthetic', g, torch.log_softmax(xs, -1).to(dev), ls, a.synthetic_beam))

    for name, g, lpd, lens, beam in cases:
        nb = int(lpd.shape[1])
        shape = dict(graph=name, states=g.num_states, arcs=len(g.src), frames=T, batch=nb, beam=beam)
        for lb in [float(v) for v in a.lattice_beams.split(',')]:
            over = wfst_lattice._decode_device(lpd.contiguous(), lens, g, beam, lb, 1.0, True, ws, to_host=False)[4]
            if int(torch.count_nonzero(over)):          # would be redone by the numpy path: minutes each
                emit(dict(lattice_beam=lb, overflowed=int(torch.count_nonzero(over)), **shape))
                continue
            batch = decode_lattice_device(lpd, lens, g, beam=beam, lattice_beam=lb, workspace_bytes=ws)[0]
            size = dict(lattice_beam=lb, nodes=batch.num_nodes, lattice_arcs=batch.num_arcs, levels=batch.num_levels,
                        nodes_per_utterance=batch.num_nodes / nb, arcs_per_utterance=batch.num_arcs / nb)
            for n in ns:
                if a.baseline_only:
                    k = min(nb, a.host_utterances)
                    t0 = time.perf_counter()
                    lats = batch.lattices()
                    t1 = time.perf_counter()
                    try:
                        lists = [lat.nbest(n) for lat in lats[:k]]
                        t2 = time.perf_counter()
                        host = (t2 - t1) * 1e3
                        emit(dict(path='lattices() + Lattice.nbest', n=n, lattices_ms=(t1 - t0) * 1e3,
                                  host_utterances=k, host_nbest_ms=host, host_nbest_ms_scaled=host * nb / k,
                                  host_ms_scaled=(t1 - t0) * 1e3 + host * nb / k,
                                  entries=sum(len(row) for row in lists), parent_checkout=parent, **size, **shape))
                    except RuntimeError as e:          # max_expansions
                        emit(dict(path='lattices() + Lattice.nbest', n=n, lattices_ms=(t1 - t0) * 1e3,
                                  host_utterances=k, error=str(e), parent_checkout=parent, **size, **shape))
                    continue
                row = dict(path='DeviceLatticeBatch.nbest', n=n, nbest_ms={}, launch_ms={}, **size, **shape)
                for th in threads:
                    lattice_dp.THREADS_PER_WORKGROUP = th
                    lists = batch.nbest(n, workspace_bytes=ws)
                    t_all = timed(lambda: batch.nbest(n, workspace_bytes=ws), a.reps)
                    t_launch = timed(lambda: (batch._nbest_launch(n, None, 1.0, ws), torch.cuda.synchronize()), a.reps)
                    row['nbest_ms'][str(th)] = t_all['median_ms']
                    row['launch_ms'][str(th)] = t_launch['median_ms']
                    row['launches'] = batch.launches
                row['entries'] = sum(len(r) for r in lists)
                best = min(row['nbest_ms'], key=row['nbest_ms'].get)
                row['best_threads'] = int(best)
                base = baseline.get((name, lb, n))
                if base and 'host_ms_scaled' in base:
                    row.update(host_ms_scaled=base['host_ms_scaled'], lattices_ms=base['lattices_ms'],
                               host_nbest_ms_scaled=base['host_nbest_ms_scaled'], host_utterances=base['host_utterances'],
                               speedup=base['host_ms_scaled'] / row['nbest_ms'][best])
                emit(row)
            del batch

if __name__ == '__main__':
    main()
