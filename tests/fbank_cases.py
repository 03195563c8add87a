"""Inputs, twins and tolerances of the feature front-end's device tests (tests/test_fbank_gpu.py,
tools/bench_fbank.py): 14 utterances whose frame counts sit on the delta clamps, the delta-delta
halo and every boundary of the kernel's 32-frame tile, in two seeded signal families, with the
numpy twin's fp64 and fp32 results.  The device tolerance is measured here, by the twin alone:
per channel, gap32 = max |twin fp32 - twin fp64|, and the device may miss the fp64 twin by 4 gap32
(the allowance for another FFT factorisation and summation order at the same precision)."""
import functools

import numpy as np

from att_speech import features as ft

FRAMES = (1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 100)
FAMILIES = ('noise', 'speech')
FACTOR = 4.0
GAP32_STATIC_MAX = 2e-4         # a degenerate input must not loosen the bound
CONFIGS = {
    # the recipes': 80 mel bins + energy, delta and delta-delta, mean-only CMVN
    'recipe': (dict(), 'mean'),
    # bench.py's 40 x 1 features
    'bench40': (dict(num_mel_bins=40, use_energy=False, delta_order=0), None),
    'small23': (dict(num_mel_bins=23, delta_order=1), 'mean_var'),
}


def utterances(family, seed=1):
    """The condition gap32_static <= 2e-4 is a property of the inputs, evaluated by the twin alone,
    and the seed was chosen under it: the Gaussian family of seed 0 holds one low-bank value 13 nats
    under its utterance's mean (pre-emphasis leaves the lowest banks 30 dB down), where the fp32
    twin itself is off by 2.03e-4."""
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    out = []
    for T in FRAMES:
        n = 400 + 160 * (T - 1) + int(rng.integers(0, 160))
        if family == 'noise':
            x = rng.standard_normal(n) * 3000.0
        else:
            t = np.arange(n) / 16000.0 + rng.uniform(0, 1)
            x = np.zeros(n)
            for f, a in zip((140, 280, 560, 980, 1700, 2500, 3400), (3000, 2200, 1500, 900, 500, 300, 150)):
                x += a * np.sin(2 * np.pi * f * t + 0.02 * f / 5.0 * np.sin(2 * np.pi * 5.0 * t) + rng.uniform(0, 6))
            x = x * (0.55 + 0.45 * np.sin(2 * np.pi * 1.3 * t)) + rng.standard_normal(n) * 30.0
        out.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return out


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def case(config='recipe', family='noise', dither=0.0, seed=0, iteration=0):
    """One batch with its twins, computed once and shared (do not modify)."""
    kw, cmvn_kind = CONFIGS[config]
    c = Case()
    utts = utterances(family)
    c.wave_lens = [len(u) for u in utts]
    c.frames = list(FRAMES)
    c.T_max = max(FRAMES)
    c.waves = np.zeros((len(utts), max(c.wave_lens)), np.int16)
    for b, u in enumerate(utts):
        c.waves[b, :len(u)] = u
    cfg = ft.make_config(dither=dither, **kw)
    F, C = ft.feat_dim(cfg), cfg.delta_order + 1
    rng = np.random.default_rng(5)
    plain64, _ = ft.fbank_batch_host(c.waves, c.wave_lens, cfg, None, np.float64, seed, iteration)
    cmvn = None
    if cmvn_kind == 'mean':
        cmvn = (rng.uniform(-5, 20, F * C).astype(np.float32), None)
    elif cmvn_kind == 'mean_var':
        import torch
        cmvn = ft.cmvn_vectors(ft.cmvn_stats(torch.from_numpy(plain64), c.frames), norm_vars=True)
    c.fe = ft.KaldiFbank(cmvn=cmvn, dither=dither, **kw)
    c.twin64, _ = ft.fbank_batch_host(c.waves, c.wave_lens, cfg, c.fe.cmvn, np.float64, seed, iteration)
    c.twin32, _ = ft.fbank_batch_host(c.waves, c.wave_lens, cfg, c.fe.cmvn, np.float32, seed, iteration)
    c.gap32 = np.abs(c.twin32.astype(np.float64) - c.twin64).max(axis=(0, 1, 2))          # per channel
    # the static gap before CMVN's scale: the condition on the inputs
    plain32, _ = ft.fbank_batch_host(c.waves, c.wave_lens, cfg, None, np.float32, seed, iteration)
    c.gap32_static = float(np.abs(plain32[..., 0].astype(np.float64) - plain64[..., 0]).max())
    return c


def errors(device_out, c):
    """per channel: max |device - twin fp64|"""
    return np.abs(np.asarray(device_out, np.float64) - c.twin64).max(axis=(0, 1, 2))
