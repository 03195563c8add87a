#!/usr/bin/env python
"""The lattice training statistics (DeviceLatticeBatch.seq_objective, csrc/lattice_train.hip) on the lattices
of tools/bench_lattice_dp.py: T' = 334, lengths uniform in [167, 334], mono o bigram / mono o trigram at 768
utterances, and the hand-made fan lattice of tests/nbest_cases.py (hub nodes with thousands of arcs).

    python tools/bench_seqtrain.py [--batch 768] [--frames 334] [--reps 20] [--rounds 3] [--lms bigram,trigram]
        [--beam 16] [--lattice-beams 2,8] [--threads 0] [--fan 3000] [--no-twin] [--twin-utterances 4] [--out FILE.json]

One JSON line per (graph, lattice beam): per quantity `rounds` windows of `reps` calls after two warm-up calls
each, the quantities alternating; the median over the windows' medians (min / max: over the windows), device
events around the whole call, every call ending in a read-back.
  mmi_ms, smbr_ms        one seq_objective call (one launch of asr_lattice_seqtrain_f64, the [T, B, C]
                         occupancies included), live scores = the decode scores plus noise
  bmmi_ms                'mmi' with a reference and boost 0.5
  posteriors_ms, frame_posteriors_ms   what the parent commit offers for the MMI occupancies: one posteriors()
                         call and one frame_posteriors() on its result (the stored scores, an index_add_ pass)
  emission_index_ms      the emission index alone, paid once per batch and [T, B, C]
  twin_ms                LatticeBatch.seq_objective('mmi') on the host over the first `--twin-utterances`
                         utterances (one call, the copy of the lattices excluded); twin_scaled_to_batch_ms: times
                         batch / that number
  max_abs_occ_diff       the launch against posteriors() + frame_posteriors() on the decode scores"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-asr_amd'), os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_wfst_decode import timed      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=768)
    ap.add_argument('--frames', type=int, default=334)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3, help='timing windows of `reps` calls per quantity, alternating')
    ap.add_argument('--lms', default='bigram,trigram')
    ap.add_argument('--beam', type=float, default=16.0)
    ap.add_argument('--lattice-beams', default='2,8')
    ap.add_argument('--workspace-mb', type=int, default=32768)
    ap.add_argument('--threads', type=int, default=0, help='lanes per workgroup of the DP kernels: 0, 64, 128, 256')
    ap.add_argument('--fan', type=int, default=3000, help='F of the fan lattice; 0: leave it out')
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--twin-utterances', type=int, default=4, help='the twin is timed on the first few utterances')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from att_speech import fst_utils as P, lattice_dp
    from att_speech.lattice_dp import DeviceLatticeBatch, decode_lattice_device
    from att_speech.wfst_decode import DecodingGraph
    from att_speech.wfst_lattice import LatticeBatch
    dev = torch.device('cuda:0')
    lattice_dp.THREADS_PER_WORKGROUP = a.threads
    golden = os.path.join(ROOT, 'tests', 'golden')
    rng = np.random.default_rng(0)
    T, B = a.frames, a.batch
    ws = a.workspace_mb << 20
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def measure(batch, lpd, shape, stored=True):
        T_, B_, C_ = lpd.shape
        live = (lpd + 0.5 * torch.rand(lpd.shape, device=dev, generator=torch.Generator(dev).manual_seed(1))).contiguous()
        ref = torch.randint(0, C_, (B_, T_), device=dev, dtype=torch.int32,
                            generator=torch.Generator(dev).manual_seed(2))
        t0 = time.perf_counter()
        batch._emission.clear()
        batch._emission_index(T_, C_)
        torch.cuda.synchronize()
        first_index_s = time.perf_counter() - t0

        def index():
            batch._emission.clear()
            batch._emission_index(T_, C_)
            torch.cuda.synchronize()
        t_index = timed(index, a.reps)
        post = batch.posteriors()
        want = post.frame_posteriors(T_, C_)
        got = batch.seq_objective(lpd, None, 'mmi')
        # only where lpd is what the lattice stores do the two compute the same thing
        diff = float((got[2] - want).abs().max()) if stored else None
        dz = float((got[0] - post.log_z)[torch.isfinite(post.log_z)].abs().max()) if stored else None
        # the two sides of the comparison alternate, `rounds` windows each: the spread is reported with them
        fns = dict(post=lambda: batch.posteriors().log_z.cpu(),
                   frames=lambda: post.frame_posteriors(T_, C_).sum().cpu(),
                   both=lambda: batch.posteriors().frame_posteriors(T_, C_).sum().cpu(),
                   mmi=lambda: batch.seq_objective(live, None, 'mmi')[2].sum().cpu(),
                   bmmi=lambda: batch.seq_objective(live, ref, 'mmi', boost=0.5)[2].sum().cpu(),
                   smbr=lambda: batch.seq_objective(live, ref, 'smbr')[2].sum().cpu())
        windows = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                windows[k].append(timed(fn, a.reps)['median_ms'])

        def med(k):
            return dict(median_ms=float(np.median(windows[k])), min_ms=min(windows[k]), max_ms=max(windows[k]))
        t_post, t_frames, t_both, t_mmi, t_bmmi, t_smbr = [med(k) for k in ('post', 'frames', 'both', 'mmi', 'bmmi',
                                                                           'smbr')]
        row = dict(threads=a.threads, nodes=batch.num_nodes, arcs=batch.num_arcs, levels=batch.num_levels,
                   emitting_arcs=batch._emission[(T_, C_)]['E'], segments=batch._emission[(T_, C_)]['S'],
                   launches=batch.launches, mmi_ms=t_mmi['median_ms'], mmi_min_ms=t_mmi['min_ms'],
                   mmi_max_ms=t_mmi['max_ms'], bmmi_ms=t_bmmi['median_ms'], smbr_ms=t_smbr['median_ms'],
                   posteriors_ms=t_post['median_ms'], frame_posteriors_ms=t_frames['median_ms'],
                   posteriors_plus_frame_posteriors_ms=t_both['median_ms'],
                   posteriors_plus_frame_posteriors_min_ms=t_both['min_ms'],
                   posteriors_plus_frame_posteriors_max_ms=t_both['max_ms'], rounds=a.rounds,
                   mmi_vs_posteriors_plus_frame_posteriors=t_mmi['median_ms'] / t_both['median_ms'],
                   emission_index_ms=t_index['median_ms'], emission_index_first_call_ms=1e3 * first_index_s,
                   max_abs_occ_diff=diff, max_abs_log_z_diff=dz, **shape)
        if not a.no_twin:
            n = min(a.twin_utterances, B_)
            hb = LatticeBatch(batch.lattices()[:n])
            lp_h, t0 = live[:, :n].cpu().numpy(), time.perf_counter()
            hb.seq_objective(lp_h, None, 'mmi')
            row['twin_utterances'] = n
            row['twin_ms'] = 1e3 * (time.perf_counter() - t0)
            row['twin_scaled_to_batch_ms'] = row['twin_ms'] * B_ / n
        emit(row)

    x = torch.from_numpy(rng.standard_normal((T, B, 49)).astype(np.float32) * 2).to(dev)
    lp = x - x.max(-1, keepdim=True)[0]
    lens_np = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    for name in [n for n in a.lms.split(',') if n]:
        gg = P.CTCGraphGen(context_order=1, num_symbols=49,
                           grammar_fst=os.path.join(golden, 'G_char_%s_syms.fst.gz' % {'bigram': 'bg', 'trigram': 'tg'}[name]),
                           vocabulary=os.path.join(golden, 'wsj_vocabulary.txt'))
        g = DecodingGraph.from_graph_generator(gg)
        for lb in [float(v) for v in a.lattice_beams.split(',')]:
            batch, redone = decode_lattice_device(lp, lens_np, g, beam=a.beam, lattice_beam=lb, workspace_bytes=ws)
            if redone:
                emit(dict(graph='mono_' + name, lattice_beam=lb, overflowed=len(redone)))
                continue
            measure(batch, lp, dict(graph='mono_' + name, lattice_beam=lb, frames=T, batch=B, beam=a.beam,
                                    states=g.num_states))
            del batch
    if a.fan > 0:
        import nbest_cases
        lat = nbest_cases.fan_lattice(a.fan)
        batch = DeviceLatticeBatch.from_lattices([lat], dev)
        lpf = torch.log_softmax(torch.randn(3, 1, 3, generator=torch.Generator().manual_seed(3)), -1).to(dev)
        measure(batch, lpf, dict(graph='fan_%d' % a.fan, lattice_beam=None, frames=3, batch=1, beam=None,
                                 states=lat.graph.num_states), stored=False)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_seqtrain.py', reps=a.reps, rows=rows), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
