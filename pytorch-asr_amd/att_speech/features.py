"""Device feature front-end: Kaldi filter-bank features, deltas and CMVN from waveforms
(csrc/fbank.hip, include/asr_amd.h: asr_fbank_f32).

The reference opens a Kaldi pipe per DataLoader worker (att_speech/data/kaldi_dataset.py:194-202;
egs/wsj/compute_features.sh:17-18: `compute-fbank-feats --use-energy=true --num-mel-bins=80 |
add-deltas`, then `apply-cmvn`).  `KaldiFbank` computes the same arithmetic in one launch and
hands `SpeechModel` its `[B, T, F, C]` fp32 input; `kaldi_fbank_host`, `add_deltas_host` and
`apply_cmvn_host` are the numpy twin of that arithmetic (fp64: the referee of the tests; fp32: the
path of CPU tensors, of configurations the launcher refuses and of ASR_FBANK_NATIVE=0).

Per frame t of an utterance of N samples (T = 1 + (N - frame_length) // frame_shift frames, the
samples taken as they are): dither, subtract the window's mean, raw log energy, pre-emphasis from
the back, Povey window, zero-pad to 512, real FFT, power of bins 0..255, mel energies, log.
Parity with the Kaldi binaries is not pinned: no Kaldi on the build machines.
"""
import collections
import os
import struct

import numpy as np
import torch

from att_speech import noise as _noise

TAG_DITHER = 2
FLT_EPSILON = float(np.finfo(np.float32).eps)
PADDED = 512
_S1 = np.array([-2., -1., 0., 1., 2.]) / 10.
DELTA_TAPS = (np.array([1.]), _S1, np.convolve(_S1, _S1))     # 1, 5 and 9 taps

_FIELDS = (('sample_frequency', 16000.), ('frame_length', 400), ('frame_shift', 160),
           ('padded', PADDED), ('num_mel_bins', 80), ('use_energy', True), ('low_freq', 20.),
           ('high_freq', 0.), ('preemph', 0.97), ('dither', 0.0), ('delta_order', 2),
           ('delta_window', 2))
FbankConfig = collections.namedtuple('FbankConfig', [f for f, _ in _FIELDS])
FbankConfig.__new__.__defaults__ = tuple(d for _, d in _FIELDS)


def make_config(**kw):
    """FbankConfig with the recipe's defaults; field types normalised so equal configurations
    are equal keys of the table cache."""
    c = FbankConfig(**kw)
    return FbankConfig(float(c.sample_frequency), int(c.frame_length), int(c.frame_shift),
                       int(c.padded), int(c.num_mel_bins), bool(c.use_energy), float(c.low_freq),
                       float(c.high_freq), float(c.preemph), float(c.dither), int(c.delta_order),
                       int(c.delta_window))


def num_frames(n_samples, config):
    """snip-edges frame count; fewer samples than one window is a ValueError"""
    n = int(n_samples)
    if n < config.frame_length:
        raise ValueError('%d samples are fewer than one window of %d' % (n, config.frame_length))
    return 1 + (n - config.frame_length) // config.frame_shift


def feat_dim(config):
    return config.num_mel_bins + (1 if config.use_energy else 0)


def native_enabled():
    """ASR_FBANK_NATIVE=0 sends KaldiFbank to the numpy twin (default: the kernel); read per call."""
    return os.environ.get('ASR_FBANK_NATIVE', '1') != '0'


# ---------------------------------------------------------------------------------------------
# tables: built in fp64, rounded once to fp32
# ---------------------------------------------------------------------------------------------
def mel_scale(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_matrix(config):
    """W [num_mel_bins, padded / 2] fp64: triangles on the mel axis over FFT bins 0..255."""
    nb, half = config.num_mel_bins, config.padded // 2
    sr = config.sample_frequency
    lo = mel_scale(config.low_freq)
    hi = mel_scale(config.high_freq if config.high_freq > 0 else sr / 2 + config.high_freq)
    delta = (hi - lo) / (nb + 1)
    m = mel_scale(np.arange(half) * sr / config.padded)
    W = np.zeros((nb, half))
    for b in range(nb):
        left = lo + b * delta
        centre, right = left + delta, left + 2 * delta
        inside = (m > left) & (m < right)
        up = (m - left) / delta
        down = (right - m) / delta
        W[b] = np.where(inside, np.where(m <= centre, up, down), 0.0)
    return W


_TABLES = {}


def tables(config):
    """The host tables of a configuration: Povey window [frame_length], twiddles
    exp(-2 pi i j / 512) as [512, 2] (cos, -sin), the dense mel matrix, and its packed form for
    the kernel: mel_idx [num_mel_bins, 3] int32 = (first bin, end bin, offset into mel_w) and
    mel_w, the weights of bins first..end-1 of every bank in turn.  'f64' holds the fp64 tables,
    'f32' the same rounded once."""
    hit = _TABLES.get(config)
    if hit is not None:
        return hit
    L, P = config.frame_length, config.padded
    i = np.arange(L, dtype=np.float64)
    window = (0.5 - 0.5 * np.cos(2 * np.pi * i / (L - 1))) ** 0.85
    j = np.arange(P, dtype=np.float64)
    tw = np.stack([np.cos(2 * np.pi * j / P), -np.sin(2 * np.pi * j / P)], -1)
    W = mel_matrix(config)
    idx = np.zeros((config.num_mel_bins, 3), np.int32)
    flat = []
    for b in range(config.num_mel_bins):
        nz = np.nonzero(W[b])[0]
        first, end = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
        idx[b] = (first, end, sum(len(f) for f in flat))
        flat.append(W[b, first:end])
    mel_w = np.concatenate(flat) if flat else np.zeros(0)
    if len(mel_w) == 0:
        mel_w = np.zeros(1)
    t64 = {'window': window, 'tw': tw, 'mel': W}
    t32 = {'window': window.astype(np.float32), 'tw': tw.astype(np.float32),
           'mel': W.astype(np.float32)}
    out = {'f64': t64, 'f32': t32, 'mel_idx': idx, 'mel_w': mel_w.astype(np.float32)}
    _TABLES[config] = out
    return out


_DEVICE_TABLES = {}


def device_tables(config, device):
    """The fp32 tables on `device`, uploaded once per (configuration, device)."""
    key = (config, str(device))
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        t = tables(config)
        hit = {'window': torch.from_numpy(t['f32']['window']).to(device),
               'tw': torch.from_numpy(t['f32']['tw']).contiguous().to(device),
               'mel_idx': torch.from_numpy(t['mel_idx']).contiguous().to(device),
               'mel_w': torch.from_numpy(t['mel_w']).to(device)}
        _DEVICE_TABLES[key] = hit
    return hit


# ---------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------
def _bit_reverse(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, np.int64)
    for k in range(bits):
        r |= ((np.arange(n) >> k) & 1) << (bits - 1 - k)
    return r


def power_spectrum(frames, tw):
    """|X_k|^2, k < 256, of the real rows `frames` [T, 512], in the rows' dtype: the even and odd
    samples form one 256-point complex sequence, a radix-2 FFT of it with the twiddles
    tw [512, 2] = exp(-2 pi i j / 512), then the split into the spectrum of the real row."""
    T, P = frames.shape
    half = P // 2
    re = frames[:, 0::2][:, _bit_reverse(half)].copy()
    im = frames[:, 1::2][:, _bit_reverse(half)].copy()
    span = 1
    while span < half:
        step = P // (2 * span)                   # exp(-2 pi i k / (2 span)) = tw[k * step]
        wr, wi = tw[0:span * step:step, 0], tw[0:span * step:step, 1]
        re = re.reshape(T, -1, 2, span)
        im = im.reshape(T, -1, 2, span)
        br = re[:, :, 1] * wr - im[:, :, 1] * wi
        bi = re[:, :, 1] * wi + im[:, :, 1] * wr
        re = np.stack([re[:, :, 0] + br, re[:, :, 0] - br], 2).reshape(T, half)
        im = np.stack([im[:, :, 0] + bi, im[:, :, 0] - bi], 2).reshape(T, half)
        span *= 2
    # Z[k], Z[(256 - k) % 256] -> X[k] = E[k] + W^k O[k]
    mirror = (half - np.arange(half)) % half
    zr, zi = re[:, mirror], -im[:, mirror]                       # conj(Z[256 - k])
    h = frames.dtype.type(0.5)
    er, ei = (re + zr) * h, (im + zi) * h
    dr, di = (re - zr) * h, (im - zi) * h                        # (Z - conj Z') / 2 = i O
    orr, oi = di, -dr                                            # O = -i (i O)
    wr, wi = tw[:half, 0], tw[:half, 1]
    xr = er + orr * wr - oi * wi
    xi = ei + orr * wi + oi * wr
    return xr * xr + xi * xi


def extract_windows(wave, config):
    """[T, frame_length] windows of one utterance, samples as they are."""
    wave = np.asarray(wave)
    T = num_frames(len(wave), config)
    idx = np.arange(T)[:, None] * config.frame_shift + np.arange(config.frame_length)[None, :]
    return wave[idx]


def kaldi_fbank_host(wave, config, dtype=np.float64, noise=None):
    """Static features [T, F] of one utterance in `dtype` (np.float64 or np.float32, every step
    in that precision with the tables of that precision).  noise: the dither draws z [T,
    frame_length], used when config.dither != 0."""
    dtype = np.dtype(dtype).type
    t = tables(config)['f64' if dtype is np.float64 else 'f32']
    L = config.frame_length
    x = extract_windows(wave, config).astype(dtype)
    if config.dither != 0.0:
        if noise is None:
            raise ValueError('dither needs its draws')
        x = x + dtype(config.dither) * np.asarray(noise).astype(dtype)
    x = x - (x.sum(axis=1, dtype=dtype) / dtype(L))[:, None]
    eps = dtype(FLT_EPSILON)
    energy = np.log(np.maximum((x * x).sum(axis=1, dtype=dtype), eps))
    p = dtype(config.preemph)
    y = x.copy()
    y[:, 1:] = x[:, 1:] - p * x[:, :-1]
    y[:, 0] = x[:, 0] - p * x[:, 0]
    y = y * t['window'][None, :]
    frames = np.zeros((len(y), config.padded), dtype)
    frames[:, :L] = y
    power = power_spectrum(frames, t['tw'])
    mel = power @ t['mel'].T
    out = np.log(np.maximum(mel, eps))
    if config.use_energy:
        out = np.concatenate([energy[:, None], out], axis=1)
    return out.astype(dtype)


def add_deltas_host(static, order=2, window=2, dtype=None):
    """static [T, F] -> [T, F, order + 1]: channel c is the sum over the taps of DELTA_TAPS[c] of
    the static frames at clamp(t + j, 0, T - 1)."""
    if window != 2 or order not in (0, 1, 2):
        raise ValueError('delta_window must be 2 and delta_order one of 0, 1, 2')
    static = np.asarray(static)
    dtype = static.dtype.type if dtype is None else np.dtype(dtype).type
    T = len(static)
    out = np.zeros(static.shape + (order + 1,), dtype)
    for c in range(order + 1):
        taps = DELTA_TAPS[c].astype(dtype)
        r = len(taps) // 2
        for k, s in enumerate(taps):
            out[:, :, c] += s * static[np.clip(np.arange(T) + k - r, 0, T - 1)].astype(dtype)
    return out


def apply_cmvn_host(feats, offset=None, scale=None):
    """feats [T, F, C]; offset, scale [F * C] in Kaldi's column order [static | delta | delta-delta]:
    y = (x - offset) * scale."""
    feats = np.asarray(feats)
    T, F, C = feats.shape
    dt = feats.dtype.type
    if offset is not None:
        feats = feats - np.asarray(offset).astype(dt).reshape(C, F).T[None]
    if scale is not None:
        feats = feats * np.asarray(scale).astype(dt).reshape(C, F).T[None]
    return feats


def dither_indices(b, T, T_max, config):
    """global noise indices ((b T_max + t) 512 + i) of utterance b's windows, [T, frame_length]"""
    t = np.arange(T, dtype=np.uint64)[:, None]
    i = np.arange(config.frame_length, dtype=np.uint64)[None, :]
    return (np.uint64(b) * np.uint64(T_max) + t) * np.uint64(PADDED) + i


def dither_draws(b, T, T_max, config, seed, iteration):
    """the draws z [T, frame_length] of utterance b in fp64 (noise.normal_f64, tag 2)"""
    idx = dither_indices(b, T, T_max, config)
    return _noise.normal_f64(idx.reshape(-1), seed, TAG_DITHER, iteration).reshape(idx.shape)


def fbank_batch_host(waves, wave_lens, config, cmvn=None, dtype=np.float32, seed=0, iteration=0,
                     t_max=None):
    """The whole front-end on the host: [B, T_max, F, C] in `dtype`, zero at t >= T_b, and the
    frame counts."""
    waves = np.asarray(waves)
    lens = [num_frames(n, config) for n in wave_lens]
    T_max = max(lens) if t_max is None else int(t_max)
    F, C = feat_dim(config), config.delta_order + 1
    out = np.zeros((len(lens), T_max, F, C), dtype)
    for b, (n, T) in enumerate(zip(wave_lens, lens)):
        z = dither_draws(b, T, T_max, config, seed, iteration) if config.dither != 0.0 else None
        static = kaldi_fbank_host(waves[b, :int(n)], config, dtype, z)
        f = add_deltas_host(static, config.delta_order, config.delta_window)
        if cmvn is not None:
            f = apply_cmvn_host(f, cmvn[0], cmvn[1])
        out[b, :T] = f
    return out, np.asarray(lens, np.int32)


# ---------------------------------------------------------------------------------------------
# the public front-end
# ---------------------------------------------------------------------------------------------
def native_supported(config):
    """asr_fbank_supported: what the launcher takes (the launcher runs the same check)"""
    from att_speech import _native
    return bool(_native.lib().asr_fbank_supported(
        config.frame_length, config.frame_shift, config.padded, config.num_mel_bins,
        config.delta_order, config.delta_window))


class KaldiFbank(object):
    """fe = KaldiFbank(num_mel_bins=80, ..., cmvn=(offset, scale) or None);
    fe(waves [B, N_max] int16 / fp32, wave_lens) -> {'features' [B, T_max, F, C] fp32,
    'features_lengths' [B] int32}.  Device tensors take the kernel; CPU tensors, configurations
    the launcher refuses and ASR_FBANK_NATIVE=0 take the fp32 twin."""

    def __init__(self, cmvn=None, **configuration):
        self.config = make_config(**configuration)
        c = self.config
        if c.padded != PADDED or not 0 < c.frame_length <= c.padded or c.frame_shift < 1:
            raise ValueError('frame_length in 1..512, frame_shift >= 1 and padded == 512')
        if c.num_mel_bins < 1 or c.delta_order not in (0, 1, 2) or c.delta_window != 2:
            raise ValueError('num_mel_bins >= 1, delta_order in 0..2, delta_window == 2')
        self.feat_dim, self.channels = feat_dim(c), c.delta_order + 1
        self.cmvn = None
        self._cmvn_dev = {}
        if cmvn is not None:
            n = self.feat_dim * self.channels
            off = np.zeros(n, np.float32) if cmvn[0] is None else np.asarray(cmvn[0], np.float32)
            sc = np.ones(n, np.float32) if cmvn[1] is None else np.asarray(cmvn[1], np.float32)
            if off.shape != (n,) or sc.shape != (n,):
                raise ValueError('cmvn vectors need %d entries' % n)
            self.cmvn = (off, sc)

    def _cmvn_on(self, device):
        if self.cmvn is None:
            return None, None
        hit = self._cmvn_dev.get(str(device))
        if hit is None:
            hit = tuple(torch.from_numpy(v).to(device) for v in self.cmvn)
            self._cmvn_dev[str(device)] = hit
        return hit

    def __call__(self, waves, wave_lens, seed=0, iteration=0, t_max=None):
        c = self.config
        if not isinstance(waves, torch.Tensor):
            waves = torch.as_tensor(np.asarray(waves))
        if waves.dim() != 2 or waves.dtype not in (torch.int16, torch.float32):
            raise TypeError('waves must be [B, N_max] int16 or float32')
        wave_lens = [int(n) for n in (wave_lens.tolist() if hasattr(wave_lens, 'tolist') else wave_lens)]
        if len(wave_lens) != waves.size(0) or any(n > waves.size(1) for n in wave_lens):
            raise ValueError('wave_lens must give B lengths within N_max')
        lens = [num_frames(n, c) for n in wave_lens]
        T_max = max(lens) if t_max is None else int(t_max)
        if T_max < max(lens):
            raise ValueError('t_max below the longest utterance')
        if c.dither != 0.0 and len(lens) * T_max * PADDED >= 1 << 34:
            raise ValueError('global noise index beyond 2^34')
        flens = torch.tensor(lens, dtype=torch.int32)
        if waves.is_cuda and native_enabled() and native_supported(c):
            feats, dev_lens = self._native(waves, wave_lens, T_max, seed, iteration)
            flens._asr_dev = (str(waves.device), flens._version, dev_lens)
        else:
            host, _ = fbank_batch_host(waves.cpu().numpy(), wave_lens, c, self.cmvn, np.float32,
                                       seed, iteration, T_max)
            feats = torch.from_numpy(host).to(waves.device)
        return {'features': feats, 'features_lengths': flens}

    def _native(self, waves, wave_lens, T_max, seed, iteration, out=None):
        from att_speech import _native
        c, dev = self.config, waves.device
        if waves.stride(1) != 1:
            waves = waves.contiguous()
        B = waves.size(0)
        tabs = device_tables(c, dev)
        off, sc = self._cmvn_on(dev)
        host_lens = torch.tensor(wave_lens, dtype=torch.int32)
        dev_lens = (host_lens.pin_memory() if B else host_lens).to(dev, non_blocking=True)
        if out is None:
            out = torch.empty((B, T_max, self.feat_dim, self.channels), dtype=torch.float32, device=dev)
        feat_lens = torch.empty(B, dtype=torch.int32, device=dev)
        _native.check(_native.lib().asr_fbank_f32(
            _native._p(waves), waves.stride(0), waves.size(1), 1 if waves.dtype == torch.int16 else 0,
            _native._p(dev_lens), B, T_max, _native._p(tabs['window']), _native._p(tabs['tw']),
            _native._p(tabs['mel_idx']), _native._p(tabs['mel_w']), tabs['mel_w'].numel(),
            c.frame_length, c.frame_shift, c.padded, c.num_mel_bins, int(c.use_energy),
            c.delta_order, c.delta_window, c.preemph, _native._p(off), _native._p(sc),
            c.dither, seed % (1 << 64), int(iteration) % (1 << 64), _native._p(out),
            _native._p(feat_lens), _native._stream()), 'asr_fbank_f32')
        return out, feat_lens


def collate_waves(waves, config=None):
    """Pad a list of 1-D sample arrays into [B, N_max] and order it by _kaldi_collate_fn's rule,
    np.argsort(frame counts)[::-1]: longest first, ties in that reversed order.  Returns
    (waves, wave_lens int64 [B], order): row r is input order[r]."""
    config = make_config() if config is None else config
    waves = [np.asarray(w) for w in waves]
    frames = [num_frames(len(w), config) for w in waves]
    order = np.argsort(frames)[::-1]
    dtype = np.result_type(*[w.dtype for w in waves])
    out = np.zeros((len(waves), max(len(w) for w in waves)), dtype)
    for r, k in enumerate(order):
        out[r, :len(waves[k])] = waves[k]
    return out, np.array([len(waves[k]) for k in order], np.int64), order


# ---------------------------------------------------------------------------------------------
# CMVN
# ---------------------------------------------------------------------------------------------
def cmvn_stats(features, lens):
    """compute-cmvn-stats of a batch: features [B, T, F, C], lens [B] -> stats [2, F C + 1] fp64 in
    Kaldi's column order: row 0 the sums and the frame count, row 1 the sums of squares and 0.
    Torch ops on the features' device."""
    B, T, F, C = features.shape
    lens = torch.as_tensor(lens).to(features.device)
    valid = (torch.arange(T, device=features.device)[None, :] < lens[:, None])
    x = features.permute(0, 1, 3, 2).reshape(B, T, C * F).double() * valid[:, :, None].double()
    stats = torch.zeros(2, C * F + 1, dtype=torch.float64, device=features.device)
    stats[0, :-1] = x.sum(dim=(0, 1))
    stats[0, -1] = valid.sum()
    stats[1, :-1] = (x * x).sum(dim=(0, 1))
    return stats


def cmvn_vectors(stats, norm_vars=False):
    """(offset, scale) fp32 of apply-cmvn: offset = mean; scale = 1, or 1 / sqrt(variance) (floored
    at 1e-20 as Kaldi does) with norm_vars."""
    stats = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    stats = stats.astype(np.float64)
    count = stats[0, -1]
    if count < 1:
        raise ValueError('CMVN statistics without frames')
    mean = stats[0, :-1] / count
    scale = np.ones_like(mean)
    if norm_vars:
        var = np.maximum(stats[1, :-1] / count - mean * mean, 1e-20)
        scale = 1.0 / np.sqrt(var)
    return mean.astype(np.float32), scale.astype(np.float32)


def write_kaldi_matrix(path, mat, binary=True):
    """One Kaldi matrix file (no key): binary float32 / float64 by the array's dtype, or text."""
    mat = np.asarray(mat)
    with open(path, 'wb') as f:
        if binary:
            mat = mat if mat.dtype == np.float32 else mat.astype(np.float64)
            f.write(b'\0B' + (b'FM ' if mat.dtype == np.float32 else b'DM '))
            f.write(b'\4' + struct.pack('<i', mat.shape[0]) + b'\4' + struct.pack('<i', mat.shape[1]))
            f.write(np.ascontiguousarray(mat).tobytes())
        else:
            rows = ['  ' + ' '.join(repr(float(v)) for v in r) for r in mat]
            f.write((' [\n' + '\n'.join(rows) + ' ]\n').encode('ascii'))


def read_cmvn(path):
    """A Kaldi CMVN statistics matrix [2, dim + 1] as fp64: text (` [ ... ]`) or binary float /
    double (the record layout of ctc_forward.KaldiFloatMatrixWriter, `FM ` or `DM `); a leading
    `key ` of an archive entry is skipped."""
    with open(path, 'rb') as f:
        data = f.read()
    pos = data.find(b'\0B')
    if 0 <= pos and b'[' not in data[:pos]:
        kind = data[pos + 2:pos + 5]
        if kind not in (b'FM ', b'DM ') or data[pos + 5:pos + 6] != b'\4' or data[pos + 10:pos + 11] != b'\4':
            raise ValueError('%s: not a Kaldi float or double matrix' % path)
        rows = struct.unpack('<i', data[pos + 6:pos + 10])[0]
        cols = struct.unpack('<i', data[pos + 11:pos + 15])[0]
        dt = np.dtype('<f4') if kind == b'FM ' else np.dtype('<f8')
        n = rows * cols * dt.itemsize
        if rows < 0 or cols < 0 or pos + 15 + n > len(data):
            raise ValueError('%s: truncated matrix' % path)
        mat = np.frombuffer(data[pos + 15:pos + 15 + n], dt).reshape(rows, cols).astype(np.float64)
    else:
        text = data.decode('ascii')
        lo, hi = text.index('['), text.rindex(']')
        rows = [r.split() for r in text[lo + 1:hi].strip().split('\n') if r.strip()]
        mat = np.array([[float(v) for v in r] for r in rows], np.float64)
    if mat.ndim != 2 or mat.shape[0] != 2 or mat.shape[1] < 2:
        raise ValueError('%s: CMVN statistics are 2 x (dim + 1), got %s' % (path, mat.shape))
    return mat
