#!/usr/bin/env python
"""Rescoring device lattices with a back-off n-gram LM (DeviceLatticeBatch.rescore_lm, asr_lattice_lmrescore_*
of csrc/lattice_lm.hip): lattices of the mono o character-bigram graph of tools/bench_mbr.py over the draws of
tools/bench_wfst_decode.py, rescored with the shipped character trigram.

    python tools/bench_lm_rescore.py [--batch 64] [--frames 100] [--reps 3] [--beam 16] [--lattice-beam 8]
        [--rescore-beam 8] [--max-lm-states 512] [--workspace-mb 8192] [--host-utterances 2]
        [--out profiles/r21_lm_rescore.json]

Two JSON lines: medians of `reps` calls after warm-up calls, device events around the whole call.
  (a) rescore         rescore_ms: the whole rescore_lm call on the device (launches, torch sorts, the graph on
                      the host); twin_ms_scaled: batch.lattices() plus the numpy twin on the first
                      --host-utterances utterances, host clock, scaled to the batch; speedup = that / rescore_ms
  (b) two_pass        bigram search + rescoring (bigram out at scale -1, trigram in) + best_paths against one
                      decode_graph over HC o trigram at the same beam: both times, how many 1-bests agree and the
                      largest cost gap
Gaussian noise is the flat worst case: every word is about as likely as any other after every history, so
the lattices grow far more under the trigram than lattices of speech do.
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--beam', type=float, default=16.0)
    ap.add_argument('--lattice-beam', type=float, default=8.0)
    ap.add_argument('--rescore-beam', type=float, default=8.0)
    ap.add_argument('--max-lm-states', type=int, default=512)
    ap.add_argument('--workspace-mb', type=int, default=8192)
    ap.add_argument('--host-utterances', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_lm_rescore.json'))
    a = ap.parse_args()
    for p in (os.path.join(ROOT, 'pytorch-asr_amd'), os.path.join(ROOT, 'tools')):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from att_speech import fst_utils as P
    from att_speech.lattice_dp import decode_lattice_device
    from att_speech.lattice_lm import BackoffLm, lm_label_map
    from att_speech.lm_fst import LmFst
    from att_speech.wfst_decode import DecodingGraph, decode_graph
    from att_speech.wfst_lattice import LatticeBatch
    from bench_wfst_decode import timed
    dev = torch.device('cuda:0')
    golden = os.path.join(ROOT, 'tests', 'golden')
    vocab = os.path.join(golden, 'wsj_vocabulary.txt')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    ws = a.workspace_mb << 20
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(dict(tool='tools/bench_lm_rescore.py', reps=a.reps, rows=rows), f, indent=1)
                f.write('\n')

    # the draws of tools/bench_wfst_decode.py, in its order
    x = torch.from_numpy(rng.standard_normal((T, B, 49)).astype(np.float32) * 2).to(dev)
    lp = x - x.max(-1, keepdim=True)[0]
    lens = rng.integers(T // 2, T + 1, size=B).astype(np.int32)

    def graph(name):
        gg = P.CTCGraphGen(context_order=1, num_symbols=49, grammar_fst=os.path.join(golden, name), vocabulary=vocab)
        return DecodingGraph.from_graph_generator(gg)
    g_bg, g_tg = graph('G_char_bg_syms.fst.gz'), graph('G_char_tg_syms.fst.gz')
    tg = LmFst.read(os.path.join(golden, 'G_char_tg_syms.fst.gz'))
    blm = BackoffLm.from_fst(tg)
    lmap = lm_label_map(tg, vocab, 49)
    kw = dict(label_map=lmap, lattice_beam=a.rescore_beam, max_lm_states=a.max_lm_states, workspace_bytes=ws)

    def search():
        return decode_lattice_device(lp, lens, g_bg, beam=a.beam, lattice_beam=a.lattice_beam, workspace_bytes=ws)

    batch, redone = search()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        res = batch.rescore_lm(blm, **kw)
    row = dict(path='DeviceLatticeBatch.rescore_lm', graph='mono_bigram', lm='char_trigram', frames=T, batch=B,
               beam=a.beam, lattice_beam=a.lattice_beam, rescore_beam=a.rescore_beam, max_lm_states=a.max_lm_states,
               redone_by_the_search=len(redone), warnings=[str(w.message) for w in caught], launches=res.launches,
               stats={k: (len(v) if isinstance(v, list) else v) for k, v in res.stats.items()})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        row['rescore_ms'] = timed(lambda: batch.rescore_lm(blm, **kw), a.reps)['median_ms']
    k = min(B, a.host_utterances)
    if k:
        t0 = time.perf_counter()
        lats = batch.lattices()
        t1 = time.perf_counter()
        twin = LatticeBatch(lats[:k]).rescore_lm(blm, label_map=lmap, lattice_beam=a.rescore_beam)
        t2 = time.perf_counter()
        scaled = (t1 - t0) * 1e3 + (t2 - t1) * 1e3 * B / k
        row.update(host_utterances=k, lattices_ms=(t1 - t0) * 1e3, twin_ms=(t2 - t1) * 1e3, twin_ms_scaled=scaled,
                   speedup=scaled / row['rescore_ms'],
                   twin_costs_agree=sum(bool(x.cost == y) for x, y in zip(twin.lattices, res.cost[:k])))
    emit(row)

    bg = BackoffLm.from_fst(LmFst.read(os.path.join(golden, 'G_char_bg_syms.fst.gz')))
    plain = dict(label_map=lmap, max_lm_states=a.max_lm_states, workspace_bytes=ws)

    def two_pass():
        b, _ = search()
        return b.rescore_lm(bg, scale=-1.0, **plain).rescore_lm(blm, **kw).best_paths()[0]

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        first = two_pass()
        t_two = timed(two_pass, a.reps)['median_ms']
        t_search = timed(search, a.reps)['median_ms']
        one = decode_graph(lp, lens, g_tg, beam=a.beam, workspace_bytes=ws)
        t_one = timed(lambda: decode_graph(lp, lens, g_tg, beam=a.beam, workspace_bytes=ws), a.reps)['median_ms']
    cost = one['cost'].cpu().numpy() if hasattr(one['cost'], 'cpu') else np.asarray(one['cost'])
    agree = sum(list(w) == list(first[b][0]) for b, w in enumerate(one['words']))
    gaps = [abs(float(cost[b]) - first[b][1]) for b in range(B) if first[b][1] < float('inf')]
    emit(dict(path='two_pass', frames=T, batch=B, beam=a.beam, lattice_beam=a.lattice_beam,
              rescore_beam=a.rescore_beam, bigram_search_ms=t_search, bigram_search_rescore_bestpath_ms=t_two,
              trigram_search_ms=t_one, trigram_graph_states=g_tg.num_states, bigram_graph_states=g_bg.num_states,
              one_bests_agree=agree, largest_cost_gap=max(gaps + [0.0]),
              trigram_search_redone_on_host=len(one['redone_on_host'])))


if __name__ == '__main__':
    main()
