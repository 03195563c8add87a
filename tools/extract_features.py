"""Waveforms to model features with the device front-end (att_speech/features.py).

  python tools/extract_features.py a.wav b.wav --out feats.npz [--cmvn stats.mat] [--norm-vars]
  python tools/extract_features.py samples.npy --out feats.npz --cpu

Inputs are 16-bit mono wav files (standard library `wave`; no resampling: the file's rate must
be the configuration's) or one .npy of samples, [N] or [B, N] int16 / float32 at full length.
Writes features [B, T_max, F, C] fp32 in the order of collate_waves (longest first),
features_lengths and that order.  --cpu runs the numpy twin instead of the kernel."""
import argparse
import os
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pytorch-asr_amd'), ROOT]


def read_wav(path, sample_frequency):
    with wave.open(path, 'rb') as w:
        if w.getnchannels() != 1 or w.getsampwidth() != 2:
            raise ValueError('%s: 16-bit mono only' % path)
        if w.getframerate() != int(sample_frequency):
            raise ValueError('%s: %d Hz, the configuration says %d (no resampling here)' % (
                path, w.getframerate(), int(sample_frequency)))
        return np.frombuffer(w.readframes(w.getnframes()), '<i2').astype(np.int16)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('inputs', nargs='+')
    ap.add_argument('--out', required=True)
    ap.add_argument('--num-mel-bins', type=int, default=80)
    ap.add_argument('--no-energy', action='store_true')
    ap.add_argument('--delta-order', type=int, default=2)
    ap.add_argument('--dither', type=float, default=0.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--sample-frequency', type=float, default=16000.0)
    ap.add_argument('--cmvn', help='Kaldi CMVN statistics matrix (text or binary)')
    ap.add_argument('--norm-vars', action='store_true')
    ap.add_argument('--cpu', action='store_true')
    args = ap.parse_args(argv)

    import torch
    from att_speech import features as ft
    if len(args.inputs) == 1 and args.inputs[0].endswith('.npy'):
        arr = np.load(args.inputs[0])
        utts = [arr] if arr.ndim == 1 else list(arr)
    else:
        utts = [read_wav(p, args.sample_frequency) for p in args.inputs]
    cmvn = None
    if args.cmvn:
        cmvn = ft.cmvn_vectors(ft.read_cmvn(args.cmvn), norm_vars=args.norm_vars)
    fe = ft.KaldiFbank(cmvn=cmvn, num_mel_bins=args.num_mel_bins, use_energy=not args.no_energy,
                       delta_order=args.delta_order, dither=args.dither,
                       sample_frequency=args.sample_frequency)
    waves, lens, order = ft.collate_waves(utts, fe.config)
    if waves.dtype not in (np.int16, np.float32):
        waves = waves.astype(np.float32)
    t = torch.from_numpy(waves)
    if not args.cpu:
        if not torch.cuda.is_available():
            raise SystemExit('no GPU: pass --cpu for the numpy twin')
        t = t.cuda()
    out = fe(t, lens, seed=args.seed)
    np.savez(args.out, features=out['features'].cpu().numpy(),
             features_lengths=out['features_lengths'].numpy(), order=np.asarray(order))
    print('%d utterances -> %s %s' % (len(utts), tuple(out['features'].shape), args.out))


if __name__ == '__main__':
    main()
