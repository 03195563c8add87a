#!/usr/bin/env python
"""Minimum-Bayes-risk decoding of lattices that stay on the device (DeviceLatticeBatch.mbr,
asr_lattice_mbr_f64 of csrc/lattice_dp.hip) at the shape of tools/bench_nbest.py: 768 utterances of
T' = 334 frames, lengths uniform in [167, 334], mono o character bigram, lattice beam 8.

    python tools/bench_mbr.py [--batch 768] [--frames 334] [--reps 3] [--beam 16] [--lattice-beams 8]
        [--threads 256] [--workspace-mb 32768] [--host-utterances 4] [--out profiles/r20_mbr.json]

One JSON line per lattice beam: medians of `reps` calls after one warm-up call, device events around
the whole call.
  mbr_ms[threads]      the whole batch.mbr() call: launches, read-back, the Python results
  launches, mean_iterations, mean_words, mean_risk
  twin_ms_scaled       LatticeBatch.mbr (numpy) on the first --host-utterances utterances, host clock,
                       plus the copy of the lattices, scaled to the batch; speedup = that / the best mbr_ms
"""
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
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--beam', type=float, default=16.0)
    ap.add_argument('--lattice-beams', default='8')
    ap.add_argument('--threads', default='256', help='lanes per workgroup to time')
    ap.add_argument('--workspace-mb', type=int, default=32768)
    ap.add_argument('--host-utterances', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r20_mbr.json'))
    a = ap.parse_args()
    for p in (os.path.join(ROOT, 'pytorch-asr_amd'), os.path.join(ROOT, 'tools')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from att_speech import fst_utils as P, lattice_dp
    from att_speech.lattice_dp import decode_lattice_device
    from att_speech.wfst_decode import DecodingGraph
    from att_speech.wfst_lattice import LatticeBatch
    from bench_wfst_decode import timed
    dev = torch.device('cuda:0')
    golden = os.path.join(ROOT, 'tests', 'golden')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    ws = a.workspace_mb << 20
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(dict(tool='tools/bench_mbr.py', reps=a.reps, rows=rows), f, indent=1)
                f.write('\n')

    # the draws of tools/bench_wfst_decode.py, in its order
    x = torch.from_numpy(rng.standard_normal((T, B, 49)).astype(np.float32) * 2).to(dev)
    lp = x - x.max(-1, keepdim=True)[0]
    lens = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    gg = P.CTCGraphGen(context_order=1, num_symbols=49, grammar_fst=os.path.join(golden, 'G_char_bg_syms.fst.gz'),
                       vocabulary=os.path.join(golden, 'wsj_vocabulary.txt'))
    g = DecodingGraph.from_graph_generator(gg)
    for lb in [float(v) for v in a.lattice_beams.split(',')]:
        batch, redone = decode_lattice_device(lp, lens, g, beam=a.beam, lattice_beam=lb, workspace_bytes=ws)
        row = dict(path='DeviceLatticeBatch.mbr', graph='mono_bigram', frames=T, batch=B, beam=a.beam, lattice_beam=lb,
                   redone_by_the_search=len(redone), nodes=batch.num_nodes, lattice_arcs=batch.num_arcs,
                   levels=batch.num_levels, nodes_per_utterance=batch.num_nodes / B,
                   arcs_per_utterance=batch.num_arcs / B, mbr_ms={})
        for th in [int(v) for v in a.threads.split(',')]:
            lattice_dp.THREADS_PER_WORKGROUP = th
            res = batch.mbr(workspace_bytes=ws)
            row['mbr_ms'][str(th)] = timed(lambda: batch.mbr(workspace_bytes=ws), a.reps)['median_ms']
            row['launches'] = batch.launches
        lattice_dp.THREADS_PER_WORKGROUP = 0
        live = [r for r in res if r.risk < float('inf')]
        row.update(mean_iterations=float(np.mean([r.iterations for r in live])),
                   mean_words=float(np.mean([len(r.words) for r in live])),
                   mean_risk=float(np.mean([r.risk for r in live])), utterances_with_a_result=len(live))
        k = min(B, a.host_utterances)
        if k:
            t0 = time.perf_counter()
            lats = batch.lattices()
            t1 = time.perf_counter()
            twin = LatticeBatch(lats[:k]).mbr()
            t2 = time.perf_counter()
            scaled = (t1 - t0) * 1e3 + (t2 - t1) * 1e3 * B / k
            best = min(row['mbr_ms'].values())
            row.update(host_utterances=k, lattices_ms=(t1 - t0) * 1e3, twin_ms=(t2 - t1) * 1e3, twin_ms_scaled=scaled,
                       speedup=scaled / best,
                       twin_words_agree=sum(x.words == y.words for x, y in zip(twin, res[:k])),
                       largest_risk_difference=max([abs(x.risk - y.risk) for x, y in zip(twin, res[:k])
                                                    if x.risk < float('inf')] + [0.0]))
        emit(row)
        del batch


if __name__ == '__main__':
    main()
