#!/usr/bin/env python
"""The lattice oracle of lattices that stay on the device (DeviceLatticeBatch.oracle, asr_lattice_oracle_i32 of
csrc/lattice_oracle.hip) at the shape of tools/bench_mbr.py: 768 utterances of T' = 334 frames, lengths uniform
in [167, 334], mono o character bigram, lattice beam 8.  The reference of an utterance is its best path with
about a tenth of the labels substituted, deleted or inserted by a seeded generator.

    python tools/bench_oracle.py [--batch 768] [--frames 334] [--reps 3] [--beam 16] [--lattice-beams 8]
        [--threads 256] [--workspace-mb 32768] [--host-utterances 4] [--noise 0.1]
        [--out profiles/r22_oracle.json]

One JSON line per lattice beam: medians of `reps` calls after two warm-up calls, device events around the whole
call.
  oracle_ms[threads]   the whole batch.oracle() call: launches, read-back, the Python results
  launches, max_words, oracle_errors, reference_words, oracle_error_rate, best_path_error_rate, mean_depth
  twin_ms_scaled       LatticeBatch.oracle (numpy) on the first --host-utterances utterances, host clock, plus
                       the copy of the lattices, SCALED to the batch; speedup = that / the best oracle_ms
  mbr_eval_ms          for orientation: batch.mbr(max_iterations=0, hypotheses=references), the single
                       evaluation of asr_lattice_mbr_f64 over the same (node x position) grid, two passes in
                       64-bit where the oracle makes one in 32-bit
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def damaged(words, rng, noise, labels):
    """the words with about `noise` of them substituted, deleted or followed by an inserted label"""
    out = []
    for w in words:
        r = rng.random()
        if r < noise / 3:
            out.append(int(rng.integers(1, labels)))
        elif r < 2 * noise / 3:
            continue
        elif r < noise:
            out += [int(w), int(rng.integers(1, labels))]
        else:
            out.append(int(w))
    return out


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]


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
    ap.add_argument('--noise', type=float, default=0.1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_oracle.json'))
    a = ap.parse_args()
    for p in (os.path.join(ROOT, 'pytorch-asr_amd'), os.path.join(ROOT, 'tools')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from att_speech import fst_utils as P, lattice_dp
    from att_speech.lattice_dp import decode_lattice_device
    from att_speech.wfst_decode import DecodingGraph
    from att_speech.wfst_lattice import LatticeBatch, oracle_error_rate
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
                json.dump(dict(tool='tools/bench_oracle.py', reps=a.reps, rows=rows), f, indent=1)
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
        best = [words for words, _, _, _ in batch.best_paths()[0]]
        noise = np.random.default_rng(1)
        refs = [damaged(words, noise, a.noise, 49) for words in best]
        row = dict(path='DeviceLatticeBatch.oracle', graph='mono_bigram', frames=T, batch=B, beam=a.beam,
                   lattice_beam=lb, redone_by_the_search=len(redone), nodes=batch.num_nodes,
                   lattice_arcs=batch.num_arcs, levels=batch.num_levels, nodes_per_utterance=batch.num_nodes / B,
                   arcs_per_utterance=batch.num_arcs / B, noise=a.noise, max_words=max(len(r) for r in refs),
                   mean_words=float(np.mean([len(r) for r in refs])), oracle_ms={})
        for th in [int(v) for v in a.threads.split(',')]:
            lattice_dp.THREADS_PER_WORKGROUP = th
            res = batch.oracle(refs, workspace_bytes=ws)
            row['oracle_ms'][str(th)] = timed(lambda: batch.oracle(refs, workspace_bytes=ws), a.reps)['median_ms']
            row['launches'] = batch.launches
        lattice_dp.THREADS_PER_WORKGROUP = 0
        total = oracle_error_rate(res, refs)
        row.update(oracle_errors=total.errors, reference_words=total.reference_words, oracle_error_rate=total.rate,
                   utterances_without_a_path=total.skipped,
                   best_path_error_rate=sum(levenshtein(w, r) for w, r in zip(best, refs)) / total.reference_words,
                   mean_depth=float(np.mean(batch.depth())))
        row['mbr_eval_ms'] = timed(lambda: batch.mbr(max_iterations=0, hypotheses=refs, workspace_bytes=ws),
                                   a.reps)['median_ms']
        row['mbr_eval_launches'] = batch.launches
        k = min(B, a.host_utterances)
        if k:
            t0 = time.perf_counter()
            lats = batch.lattices()
            t1 = time.perf_counter()
            twin = LatticeBatch(lats[:k]).oracle(refs[:k])
            t2 = time.perf_counter()
            scaled = (t1 - t0) * 1e3 + (t2 - t1) * 1e3 * B / k
            fastest = min(row['oracle_ms'].values())
            row.update(host_utterances=k, lattices_ms=(t1 - t0) * 1e3, twin_ms=(t2 - t1) * 1e3, twin_ms_scaled=scaled,
                       speedup=scaled / fastest, twin_results_agree=sum(x == y for x, y in zip(twin, res[:k])))
        emit(row)
        del batch


if __name__ == '__main__':
    main()
