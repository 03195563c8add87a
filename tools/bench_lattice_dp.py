#!/usr/bin/env python
"""The acoustic-scale sweep and the posteriors over lattices that stay on the device
(att_speech.lattice_dp, csrc/lattice_dp.hip) on the inputs of tools/bench_wfst_lattice.py: T' = 334,
lengths uniform in [167, 334]; mono o bigram / mono o trigram at 768 utterances, a synthetic graph of
about `--synthetic-states` states at 16.

    python tools/bench_lattice_dp.py [--batch 768] [--frames 334] [--reps 5] [--lms bigram,trigram]
        [--beam 16] [--lattice-beams 2,8] [--synthetic-states 1000000] [--synthetic-batch 16]
        [--threads 0] [--parent-json FILE[,FILE...]] [--out FILE.json]

One JSON line per (graph, lattice beam): medians of `reps` calls after two warm-up calls, device
events around the whole call, every call ending in a read-back.
  sweep_ms     decode_lattice_device + one best_paths call over ten acoustic scales 1.0 .. 0.1
  search_ms    decode_lattice_device without its level build (the launch, the canonical sort, the
               packing on the device)
  levels_ms    the level structure alone (DeviceLatticeBatch._build_levels)
  dp_ms        the one best_paths call (launch, read-back of costs and words, the word lists)
  ten_decode_graph_ms   ten decode_graph calls at those scales, this commit
  same_words_as_ten_searches   share of (utterance, scale) pairs with the fresh search's words
  posteriors_ms, frame_posteriors_ms   one posteriors() call, one frame_posteriors() on its result
--parent-json: --out files of tools/bench_wfst_lattice.py run from a checkout of the parent commit
in the same job (the same seed draws the same inputs); their acwt_sweep rows give the baselines
parent_lattice_ten_best_paths_ms (one decode_lattice + ten LatticeBatch.best_paths on the host) and
parent_ten_decode_graph_ms per (graph, lattice beam)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-asr_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_wfst_decode import synthetic_graph, timed      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=768)
    ap.add_argument('--frames', type=int, default=334)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lms', default='bigram,trigram')
    ap.add_argument('--beam', type=float, default=16.0)
    ap.add_argument('--lattice-beams', default='2,8')
    ap.add_argument('--synthetic-states', type=int, default=1000000)
    ap.add_argument('--synthetic-batch', type=int, default=16)
    ap.add_argument('--synthetic-beam', type=float, default=16.0)
    ap.add_argument('--synthetic-classes', type=int, default=200)
    ap.add_argument('--workspace-mb', type=int, default=32768)
    ap.add_argument('--decode-workspace-mb', type=int, default=8192)
    ap.add_argument('--threads', type=int, default=0, help='lanes per workgroup of the DP kernels: 0, 64, 128, 256')
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from att_speech import fst_utils as P, lattice_dp, wfst_lattice
    from att_speech.lattice_dp import decode_lattice_device
    from att_speech.wfst_decode import DecodingGraph, decode_graph
    dev = torch.device('cuda:0')
    lattice_dp.THREADS_PER_WORKGROUP = a.threads
    golden = os.path.join(ROOT, 'tests', 'golden')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    ws, dws = a.workspace_mb << 20, a.decode_workspace_mb << 20
    parent = {}
    for path in [p for p in (a.parent_json or '').split(',') if p]:
        for r in json.load(open(path))['rows']:
            if r['search'] == 'acwt_sweep':
                parent[(r['graph'], float(r['lattice_beam']))] = (r['one_lattice_ten_best_paths_ms'],
                                                                  r['ten_decode_graph_ms'])
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

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

    scales = [round(1.0 - 0.1 * i, 1) for i in range(10)]
    for name, g, lpd, lens, beam in cases:
        shape = dict(graph=name, states=g.num_states, arcs=len(g.src), frames=T, batch=int(lpd.shape[1]), beam=beam)

        def sweep_search():
            return [decode_graph(lpd, lens, g, beam=beam, acoustic_scale=s, workspace_bytes=dws) for s in scales]
        ten = sweep_search()
        t10 = timed(sweep_search, a.reps)
        for lb in [float(v) for v in a.lattice_beams.split(',')]:
            over = wfst_lattice._decode_device(lpd.contiguous(), lens, g, beam, lb, 1.0, True, ws, to_host=False)[4]
            if int(torch.count_nonzero(over)):          # would be redone by the numpy path: minutes each
                emit(dict(search='device_sweep', lattice_beam=lb, overflowed=int(torch.count_nonzero(over)),
                          workspace_mb=a.workspace_mb, **shape))
                continue

            def search():
                return decode_lattice_device(lpd, lens, g, beam=beam, lattice_beam=lb, workspace_bytes=ws)[0]

            def search_only():
                out = wfst_lattice._decode_device(lpd.contiguous(), lens, g, beam, lb, 1.0, True, ws, to_host=False)
                return [t.cpu() for t in out[:5]]

            def sweep():
                return search().best_paths(scales)
            batch = search()
            one = batch.best_paths(scales)
            same = np.mean([[o[b][0] == t['words'][b] for b in range(len(lens))] for o, t in zip(one, ten)])
            t_sweep = timed(sweep, a.reps)
            t_search = timed(search_only, a.reps)
            t_levels = timed(lambda: (batch._build_levels(), torch.cuda.synchronize()), a.reps)
            t_dp = timed(lambda: batch.best_paths(scales), a.reps)
            post = batch.posteriors()
            t_post = timed(lambda: batch.posteriors().log_z.cpu(), a.reps)
            t_frames = timed(lambda: post.frame_posteriors().sum().cpu(), a.reps)
            frames = float(np.sum(lens))
            base = parent.get((name, lb), (None, None))
            emit(dict(search='device_sweep', lattice_beam=lb, scales=scales, threads=a.threads,
                      nodes_per_frame=batch.num_nodes / frames, arcs_per_frame=batch.num_arcs / frames,
                      levels=batch.num_levels, launches=batch.launches,
                      sweep_ms=t_sweep['median_ms'], sweep_min_ms=t_sweep['min_ms'], sweep_max_ms=t_sweep['max_ms'],
                      search_ms=t_search['median_ms'], levels_ms=t_levels['median_ms'], dp_ms=t_dp['median_ms'],
                      ten_decode_graph_ms=t10['median_ms'], sweep_vs_ten_decode_graph=t_sweep['median_ms'] / t10['median_ms'],
                      parent_lattice_ten_best_paths_ms=base[0], parent_ten_decode_graph_ms=base[1],
                      sweep_vs_parent_lattice=t_sweep['median_ms'] / base[0] if base[0] else None,
                      sweep_vs_parent_ten_decode_graph=t_sweep['median_ms'] / base[1] if base[1] else None,
                      same_words_as_ten_searches=float(same),
                      posteriors_ms=t_post['median_ms'], frame_posteriors_ms=t_frames['median_ms'], **shape))
            del batch, post, one
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_lattice_dp.py', reps=a.reps, rows=rows), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
