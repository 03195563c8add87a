"""Times the device feature front-end (att_speech.features.KaldiFbank, csrc/fbank.hip) at
768 x 1000 frames for the recipes' configuration (80 mel + energy, deltas, mean CMVN ->
[768, 1000, 81, 3]) and for bench.py's 40 x 1 shape, and records the accuracy ratios of
tests/test_fbank_gpu.py (device error over the fp32 twin's, per channel; the tests allow 4).

Baselines, both named for what they are:
  * the numpy fp32 twin in one process, timed on a few utterances and SCALED to the batch;
  * the WSJ-shape training step of the parent commit: the kernel time per step summed from
    profiles/r03_wsj_b768_kernel_stats.csv (its 8 steps = the backward LSTM's calls / 4 layers).
Writes profiles/r27_fbank.json (--out).  Needs the MI355X; there is no pass mark on the times."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pytorch-asr_amd'), os.path.join(ROOT, 'tests'), ROOT]

HBM_PEAK = 8.0e12           # bytes/s, the MI355X's HBM3E specification
SHAPES = {'recipe': dict(), 'bench40': dict(num_mel_bins=40, use_energy=False, delta_order=0)}


def timed(fn, n):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def wsj_step_seconds(path):
    total, steps = 0, None
    with open(path) as f:
        for row in csv.DictReader(f):
            total += int(row['TotalDurationNs'])
            if 'lstm_bwd_persist_kernel' in row['Name']:
                steps = int(row['Calls']) // 4
    return total * 1e-9 / steps, steps


def accuracy_ratios():
    import torch
    import fbank_cases as fc
    out = {}
    for config in fc.CONFIGS:
        for family in fc.FAMILIES:
            c = fc.case(config, family)
            got = c.fe(torch.from_numpy(c.waves).cuda(), c.wave_lens)['features'].cpu().numpy()
            err = fc.errors(got, c)
            out['%s/%s' % (config, family)] = {'err': err.tolist(), 'gap32': c.gap32.tolist(),
                                               'ratio': (err / c.gap32).tolist(),
                                               'gap32_static': c.gap32_static}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=768)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--twin-utterances', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r27_fbank.json'))
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from att_speech import features as ft
    assert torch.cuda.is_available(), 'bench_fbank.py measures on the MI355X'
    dev = torch.device('cuda:0')
    B, T = args.batch, args.frames
    N = 400 + 160 * (T - 1)
    g = torch.Generator(device=dev).manual_seed(0)
    waves = (torch.randn(B, N, device=dev, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16)
    lens = [N] * B
    step, steps = wsj_step_seconds(os.path.join(ROOT, 'profiles', 'r03_wsj_b768_kernel_stats.csv'))
    result = {'device': torch.cuda.get_device_name(0), 'batch': B, 'frames': T, 'samples': N,
              'audio_seconds': B * N / 16000.0, 'hbm_peak_bytes_per_s': HBM_PEAK,
              'wsj_step_kernel_seconds': step, 'wsj_step_source': 'r03_wsj_b768_kernel_stats.csv, %d steps' % steps,
              'shapes': {}}
    for name, kw in SHAPES.items():
        cfg = ft.make_config(**kw)
        F, C = ft.feat_dim(cfg), cfg.delta_order + 1
        cmvn = (np.random.default_rng(1).uniform(-5, 20, F * C).astype(np.float32), None) if name == 'recipe' else None
        fe = ft.KaldiFbank(cmvn=cmvn, **kw)
        out = torch.empty(B, T, F, C, device=dev)
        call = timed(lambda: fe(waves, lens), args.iters)                              # the public call
        launch = timed(lambda: fe._native(waves, lens, T, 0, 0, out=out), args.iters)   # into a kept buffer
        small = waves[:args.twin_utterances].cpu().numpy()
        t0 = time.perf_counter()
        ft.fbank_batch_host(small, lens[:args.twin_utterances], cfg, fe.cmvn, np.float32)
        twin = (time.perf_counter() - t0) / args.twin_utterances * B
        moved = waves.numel() * 2 + out.numel() * 4
        result['shapes'][name] = {
            'output': [B, T, F, C], 'call_seconds': call, 'launch_seconds': launch,
            'bytes_moved': moved, 'hbm_fraction': moved / launch / HBM_PEAK,
            'times_real_time': B * N / 16000.0 / launch,
            'twin_fp32_seconds_scaled': twin,
            'twin_note': 'numpy fp32 twin, one process, %d utterances timed and scaled to %d' % (args.twin_utterances, B),
            'share_of_wsj_step': launch / step}
        print('%-8s call %.3f ms  launch %.3f ms  %.2f TB/s (%.0f %% of HBM peak)  twin (scaled) %.1f s' % (
            name, call * 1e3, launch * 1e3, moved / launch / 1e12, 100 * moved / launch / HBM_PEAK, twin))
    result['accuracy'] = accuracy_ratios()
    worst = max(max(v['ratio']) for v in result['accuracy'].values())
    print('worst err / gap32 ratio %.2f (the tests allow 4)' % worst)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
