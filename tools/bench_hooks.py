"""What the recipes' full hook set costs per training step (egs/wsj/yamls/ctc.yaml:90-103:
GradientClipping, KillOnNan, LinearIncreaseWeightNoise, PolyakDecay), at bench.py's workload
(mono-char CTC, 768 utterances x 1000 frames on one GPU) and warm-up.  ms/step of
att_speech.dp.train_step with

  bench_hooks:        bench.py's hooks (clipping + Polyak), device step boundary (FusedClipAdam);
  recipe_fused:       the full set at an iteration past start_iteration (sigma = 0.15 on every
                      noised weight), device noise kernel, KillOnNan in device mode;
  recipe_torch_host:  the same set with ASR_NATIVE_NOISE=0 (torch noise) and KillOnNan in host
                      mode (a loss read-back per step); the clip / Adam boundary stays on the device.

and the time of one noise launch (csrc/noise.hip, apply over every noised weight) against
8 bytes x noised elements / 8 TB/s.  Prints one JSON line.

    python tools/bench_hooks.py [--steps 20] [--warmup 5]"""
import argparse
import contextlib
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-asr_amd')]

import torch  # noqa: E402

import bench  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=768)
    ap.add_argument('--frames', type=int, default=1000)
    a = ap.parse_args()
    from att_speech import noise
    from att_speech.dp import FlatGradBucket, train_step
    from att_speech.fused_step import FusedClipAdam
    from att_speech.models import SpeechModel
    from att_speech.modules.hooks import (GradientClipping, KillOnNan, LinearIncreaseWeightNoise,
                                          PolyakDecay)
    bench.pin_gemm_selection(0)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    B, T = a.batch, a.frames
    feats, lens, texts, llens = bench.synthetic_batch(B, T, 0, 1)
    enc_cfg, dec_cfg = bench.model_config(1)
    torch.manual_seed(1234)
    sb = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(), 'spkids': None}
    model0 = SpeechModel(enc_cfg, dec_cfg, sb, bench.S, [str(i) for i in range(bench.S)]).to(dev)
    feats_d = feats.to(dev)
    clip_scale = B / 16.0           # bench.py's thresholds for a summed loss over B utterances
    start_it = 20000

    def run(name, recipe, device_kill, native_noise):
        os.environ['ASR_NATIVE_NOISE'] = '1' if native_noise else '0'
        model = copy.deepcopy(model0)
        bucket = FlatGradBucket(model.parameters())
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        hooks = [GradientClipping(clip_norm=10000.0 * clip_scale, skip_step_norm=100000.0 * clip_scale),
                 PolyakDecay(decay_rates=[0.9998])]
        kill = None
        if recipe:
            kill = KillOnNan(priority=5)
            hooks = sorted(hooks + [LinearIncreaseWeightNoise(
                start_iteration=start_it, weight_noise={'decoder': 0.15, 'encoder': 0.15}), kill],
                key=lambda h: h.priority)
        for h in hooks:
            h.pre_run(model, opt)
        fused = FusedClipAdam.from_optimizer(opt, bucket, hooks[0],
                                             kill_on_nan=kill if device_kill else None)
        host_skips = []

        def step(it):
            with contextlib.redirect_stdout(sys.stderr):
                _, skip = train_step(model, opt, ((feats_d, lens, None, texts, llens), {}), hooks=hooks,
                                     bucket=bucket, current_iteration=it, fused=fused)
            host_skips.append(bool(skip))
        it = start_it + 1
        for _ in range(a.warmup):
            step(it)
            it += 1
            torch.cuda.synchronize()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(a.steps):
            step(it)
            it += 1
        torch.cuda.synchronize()
        dt = time.time() - t0
        recs = fused.drain()[-a.steps:]
        skipped = sum(h or r[2] for h, r in zip(host_skips[-a.steps:], recs))
        res = {'ms_per_step': dt / a.steps * 1e3, 'skipped_steps': int(skipped)}
        del model, bucket, opt, fused
        torch.cuda.empty_cache()
        return name, res

    out = dict(run(*c) for c in (('bench_hooks', False, False, True),
                                 ('recipe_fused', True, True, True),
                                 ('recipe_torch_host', True, False, False)))
    os.environ['ASR_NATIVE_NOISE'] = '1'
    base = out['bench_hooks']['ms_per_step']
    for k in ('recipe_fused', 'recipe_torch_host'):
        out[k]['overhead_pct'] = (out[k]['ms_per_step'] / base - 1) * 100

    # one apply launch over every noised weight of the model
    hook = LinearIncreaseWeightNoise(start_iteration=start_it, weight_noise=0.15, seed=1)
    params = [(n, p) for n, p in model0.named_parameters() if hook._requires_noise(n)]
    ws = [p for _, p in params]
    starts, s = [], 0
    for p in ws:
        starts.append(s)
        s += p.numel()
    tab = noise.SegmentTable()
    table, nsegs = tab.get(ws, starts, [0.15] * len(ws))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = 50
    for sign in (1, -1):
        noise.launch(table, nsegs, 1, noise.TAG_WEIGHT, 5, sign=sign)
    ev[0].record()
    for r in range(reps):
        noise.launch(table, nsegs, 1, noise.TAG_WEIGHT, 5, sign=1 if r % 2 == 0 else -1)
    ev[1].record()
    torch.cuda.synchronize()
    us = ev[0].elapsed_time(ev[1]) / reps * 1e3
    floor_us = 8.0 * s / HBM_BYTES_PER_S * 1e6
    out['noise_apply'] = {'noised_elements': s, 'segments': nsegs, 'us_per_launch': us,
                          'hbm_floor_us': floor_us, 'fraction_of_floor': floor_us / us}
    out.update(workload='mono-char CTC, %d x %d frames, 1 GPU, iteration > start_iteration' % (B, T),
               steps=a.steps, warmup=a.warmup)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
