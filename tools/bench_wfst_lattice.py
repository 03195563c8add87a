#!/usr/bin/env python
"""Lattice generation (att_speech.wfst_lattice.decode_lattice, csrc/wfst_lattice.hip) against the
1-best search (decode_graph) on the inputs of tools/bench_wfst_decode.py: T' = 334, lengths uniform
in [167, 334]; mono o bigram / mono o trigram at 768 utterances, a synthetic graph of about
`--synthetic-states` states at 16.

    python tools/bench_wfst_lattice.py [--batch 768] [--frames 334] [--reps 5] [--lms bigram,trigram]
        [--beam 16] [--lattice-beams 2,8] [--synthetic-states 1000000] [--synthetic-batch 16]
        [--synthetic-beam 16] [--parent-json FILE] [--out FILE.json]

One JSON line per measurement: median, min and max of `reps` calls after two warm-up calls, device
events around the whole call (launch, read-back of the kept nodes and arcs, the host's sort into
the canonical form).  `kernel_ms` is the launch alone, `device_ms` the launch plus the sort into the
canonical order on the device and the copy to the host, so the shares can be read off.  Per lattice beam: the nodes and arcs kept per frame.  The sweep row: one
decode_lattice plus ten best-path re-rankings (LatticeBatch.best_paths, acoustic scales 1.0 down to
0.1) against ten decode_graph calls at those scales, and how many of the 1-best word sequences
agree.  --parent-json: the --out file of tools/bench_wfst_decode.py run from a checkout of the
parent commit on the same machine (it draws the same inputs from the same seed); its decode_graph
medians are copied in as `parent_decode_ms`."""
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
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from att_speech import fst_utils as P, wfst_lattice
    from att_speech.wfst_decode import DecodingGraph, decode_graph
    from att_speech.wfst_lattice import LatticeBatch, decode_lattice
    dev = torch.device('cuda:0')
    golden = os.path.join(ROOT, 'tests', 'golden')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    ws, dws = a.workspace_mb << 20, a.decode_workspace_mb << 20
    parent = {}
    if a.parent_json:
        for r in json.load(open(a.parent_json))['rows']:
            if r['search'] == 'beam':
                parent[(r['graph'], float(r['beam']))] = r['median_ms']
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
        dec = timed(lambda: decode_graph(lpd, lens, g, beam=beam, workspace_bytes=dws), a.reps)
        emit(dict(search='decode_graph', parent_decode_ms=parent.get((name, beam)), **shape, **dec))
        frames = float(np.sum(lens))
        usable = True
        for lb in [float(v) for v in a.lattice_beams.split(',')]:
            # an utterance that outgrows the workspace is redone by the numpy path, minutes each at
            # these sizes: look at the flags first and leave the row out when that would happen
            over = int(np.count_nonzero(wfst_lattice._decode_device(lpd.contiguous(), lens, g, beam, lb, 1.0, True, ws)[4]))
            if over:
                usable = False
                emit(dict(search='decode_lattice', lattice_beam=lb, overflowed=over, workspace_mb=a.workspace_mb, **shape))
                continue
            lats, redone = decode_lattice(lpd, lens, g, beam=beam, lattice_beam=lb, workspace_bytes=ws)
            t = timed(lambda: decode_lattice(lpd, lens, g, beam=beam, lattice_beam=lb, workspace_bytes=ws), a.reps)
            d = timed(lambda: wfst_lattice._decode_device(lpd.contiguous(), lens, g, beam, lb, 1.0, True, ws), a.reps)
            k = timed(lambda: wfst_lattice._decode_device(lpd.contiguous(), lens, g, beam, lb, 1.0, True, ws, pack=False),
                      a.reps)
            base = parent.get((name, beam))
            emit(dict(search='decode_lattice', lattice_beam=lb, redone_on_host=len(redone),
                      nodes_per_frame=sum(l.num_nodes for l in lats) / frames,
                      arcs_per_frame=sum(l.num_arcs for l in lats) / frames,
                      kernel_ms=k['median_ms'], kernel_vs_decode_graph=k['median_ms'] / dec['median_ms'],
                      device_ms=d['median_ms'], vs_decode_graph=t['median_ms'] / dec['median_ms'],
                      device_vs_decode_graph=d['median_ms'] / dec['median_ms'],
                      vs_parent_decode_graph=t['median_ms'] / base if base else None, **shape, **t))
        if not usable:
            continue
        lb = float(a.lattice_beams.split(',')[-1])

        def sweep_lattice():
            batch = LatticeBatch(decode_lattice(lpd, lens, g, beam=beam, lattice_beam=lb, workspace_bytes=ws)[0])
            return [batch.best_paths(acoustic_scale=s) for s in scales]

        def sweep_search():
            return [decode_graph(lpd, lens, g, beam=beam, acoustic_scale=s, workspace_bytes=dws) for s in scales]
        one, ten = sweep_lattice(), sweep_search()
        same = np.mean([[o[b][0] == t10['words'][b] for b in range(len(lens))] for o, t10 in zip(one, ten)])
        t1, t10 = timed(sweep_lattice, a.reps), timed(sweep_search, a.reps)
        emit(dict(search='acwt_sweep', lattice_beam=lb, scales=scales, one_lattice_ten_best_paths_ms=t1['median_ms'],
                  ten_decode_graph_ms=t10['median_ms'], ratio=t1['median_ms'] / t10['median_ms'],
                  same_words_as_ten_searches=float(same), **shape))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_wfst_lattice.py', reps=a.reps, rows=rows), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
