"""The feature front-end's host side (att_speech/features.py): the numpy twin of the filter-bank,
delta and CMVN arithmetic against slow independent statements, the tables, batching and the
argument checks of asr_fbank_f32.  No GPU."""
import numpy as np
import pytest
import torch

from att_speech import _native, features as ft

CFG = ft.make_config()
LOG_EPS = float(np.log(np.float64(ft.FLT_EPSILON)))


def _wave(n, seed=0, scale=3000.0):
    return np.round(np.random.default_rng(seed).standard_normal(n) * scale).astype(np.int16)


def test_fft_and_power_match_a_direct_dft():
    """the fp64 twin's FFT and power stage against an O(N^2) DFT with a cosine / sine matrix"""
    T = 9
    wave = _wave(400 + 160 * (T - 1) + 37, seed=1).astype(np.float64)
    x = ft.extract_windows(wave, CFG)
    x = x - x.mean(axis=1, keepdims=True)
    y = x.copy()
    y[:, 1:] = x[:, 1:] - CFG.preemph * x[:, :-1]
    y[:, 0] = x[:, 0] - CFG.preemph * x[:, 0]
    frames = np.zeros((T, 512))
    frames[:, :400] = y * ft.tables(CFG)['f64']['window']
    n, k = np.arange(512)[:, None], np.arange(256)[None, :]
    ang = 2 * np.pi * n * k / 512
    want = (frames @ np.cos(ang)) ** 2 + (frames @ np.sin(ang)) ** 2
    got = ft.power_spectrum(frames, ft.tables(CFG)['f64']['tw'])
    assert got.shape == (T, 256)
    err = np.abs(got - want).max(axis=1) / want.sum(axis=1)
    assert err.max() <= 1e-9, err


@pytest.mark.parametrize('kw', [{}, {'num_mel_bins': 40}, {'num_mel_bins': 23}])
def test_mel_table(kw):
    cfg = ft.make_config(**kw)
    W = ft.tables(cfg)['f64']['mel']
    assert W.shape == (cfg.num_mel_bins, 256)
    assert (W >= 0).all() and W.max() <= 1.0 and (W.max(axis=1) > 0).all()
    for k in range(256):
        banks = np.nonzero(W[:, k])[0]
        assert len(banks) <= 2
        if len(banks) == 2:
            assert banks[1] == banks[0] + 1
            assert abs(W[banks, k].sum() - 1.0) <= 1e-12
    below = np.arange(256) * cfg.sample_frequency / 512 <= cfg.low_freq
    assert below[0] and (W[:, below] == 0).all()
    # the packed form the kernel reads is the dense matrix
    idx, w = ft.tables(cfg)['mel_idx'], ft.tables(cfg)['mel_w']
    dense = np.zeros_like(W, dtype=np.float32)
    for b, (first, end, off) in enumerate(idx):
        assert 0 <= first <= end <= 256 and off + end - first <= len(w)
        dense[b, first:end] = w[off:off + end - first]
    assert (dense == W.astype(np.float32)).all()


def test_frame_count():
    with pytest.raises(ValueError):
        ft.num_frames(399, CFG)
    with pytest.raises(ValueError):
        ft.KaldiFbank()(torch.zeros(1, 399), [399])
    assert [ft.num_frames(n, CFG) for n in (400, 559, 560)] == [1, 1, 2]
    for n, T in ((400, 1), (559, 1), (560, 2)):
        got = ft.KaldiFbank()(torch.zeros(1, n), [n])
        assert got['features'].shape == (1, T, 81, 3)
        assert got['features_lengths'].tolist() == [T] and got['features_lengths'].dtype == torch.int32


def test_all_zero_signal_gives_log_epsilon():
    for dtype in (np.float64, np.float32):
        got = ft.kaldi_fbank_host(np.zeros(1000, np.int16), CFG, dtype)
        assert got.shape == (4, 81) and got.dtype == dtype
        assert np.abs(got - LOG_EPS).max() <= 2e-6


def test_sinusoid_peaks_in_its_bank():
    nb = CFG.num_mel_bins
    lo, hi = ft.mel_scale(CFG.low_freq), ft.mel_scale(CFG.sample_frequency / 2)
    centre_mel = lo + (40 + 1) * (hi - lo) / (nb + 1)
    freq = 700.0 * (np.exp(centre_mel / 1127.0) - 1.0)
    wave = 8000.0 * np.sin(2 * np.pi * freq * np.arange(4000) / CFG.sample_frequency)
    got = ft.kaldi_fbank_host(wave.astype(np.float32), CFG)
    assert (np.argmax(got[:, 1:], axis=1) == 40).all()


def test_deltas():
    T, F = 20, 5
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(F), rng.standard_normal(F)
    ramp = a[None, :] * np.arange(T)[:, None] + b[None, :]
    d = ft.add_deltas_host(ramp, 2)
    assert d.shape == (T, F, 3)
    assert np.array_equal(d[:, :, 0], ramp)
    assert np.abs(d[4:T - 4, :, 1] - a).max() <= 1e-12
    assert np.abs(d[4:T - 4, :, 2]).max() <= 1e-12
    one = ft.add_deltas_host(ramp[:1], 2)
    assert np.abs(one[:, :, 1:]).max() <= 1e-12
    assert ft.add_deltas_host(ramp, 0).shape == (T, F, 1)
    # every frame, the edges among them, against the clamped sum written as a loop
    static = rng.standard_normal((11, F))
    s1 = [-0.2, -0.1, 0.0, 0.1, 0.2]
    s2 = [0.04, 0.04, 0.01, -0.04, -0.1, -0.04, 0.01, 0.04, 0.04]
    got = ft.add_deltas_host(static, 2)
    for t in range(11):
        for f in range(F):
            d1 = sum(s1[j + 2] * static[min(max(t + j, 0), 10), f] for j in range(-2, 3))
            d2 = sum(s2[j + 4] * static[min(max(t + j, 0), 10), f] for j in range(-4, 5))
            assert abs(got[t, f, 1] - d1) <= 1e-12 and abs(got[t, f, 2] - d2) <= 1e-12
    # delta-delta is the delta of the unclamped delta: the 9 taps are s1 * s1
    assert np.abs(ft.DELTA_TAPS[2] - np.array(s2)).max() <= 1e-15


def test_cmvn_statistics_and_files(tmp_path):
    rng = np.random.default_rng(3)
    B, T, F, C = 3, 17, 6, 3
    lens = [17, 9, 4]
    x = torch.from_numpy(rng.standard_normal((B, T, F, C)) * 3 + 5).float()
    stats = ft.cmvn_stats(x, lens)
    assert stats.shape == (2, F * C + 1) and stats.dtype == torch.float64
    assert float(stats[0, -1]) == sum(lens)
    valid = np.concatenate([x[b, :n].numpy() for b, n in enumerate(lens)])       # [frames, F, C]
    for norm_vars in (False, True):
        off, scale = ft.cmvn_vectors(stats, norm_vars)
        y = ft.apply_cmvn_host(valid.astype(np.float64), off, scale)
        assert np.abs(y.mean(axis=0)).max() <= 1e-5
        if norm_vars:
            assert np.abs(y.var(axis=0) - 1.0).max() <= 1e-4
        else:
            assert (scale == 1).all()
    # Kaldi's column order: entry c F + f
    assert abs(float(stats[0, 1 * F + 2]) - valid[:, 2, 1].astype(np.float64).sum()) <= 1e-6 * sum(lens) * 10
    mat = stats.numpy()
    for name, binary, m in (('t.txt', False, mat), ('d.bin', True, mat), ('f.bin', True, mat.astype(np.float32))):
        path = str(tmp_path / name)
        ft.write_kaldi_matrix(path, m, binary=binary)
        back = ft.read_cmvn(path)
        assert back.dtype == np.float64 and np.array_equal(back, m.astype(np.float64))
    ft.write_kaldi_matrix(str(tmp_path / 'bad'), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        ft.read_cmvn(str(tmp_path / 'bad'))


def test_collate_and_padding():
    ns = [400 + 160 * 4 + 3, 400 + 160 * 9, 400 + 160 * 4 + 77, 400, 400 + 160 * 9 + 159]
    waves = [_wave(n, seed=10 + k) for k, n in enumerate(ns)]
    batch, lens, order = ft.collate_waves(waves)
    frames = [ft.num_frames(n, CFG) for n in ns]
    assert list(order) == list(np.argsort(frames)[::-1]) == [4, 1, 2, 0, 3]
    assert batch.shape == (5, max(ns)) and batch.dtype == np.int16
    assert list(lens) == [ns[k] for k in order]
    for r, k in enumerate(order):
        assert np.array_equal(batch[r, :ns[k]], waves[k]) and not batch[r, ns[k]:].any()
    fe = ft.KaldiFbank()
    a = fe(torch.from_numpy(batch), lens)
    dirty = batch.copy()
    for r, n in enumerate(lens):
        dirty[r, n:] = 12345
    b = fe(torch.from_numpy(dirty), lens)
    assert torch.equal(a['features'], b['features'])
    assert a['features_lengths'].tolist() == [frames[k] for k in order]
    for r, k in enumerate(order):
        assert (a['features'][r, frames[k]:] == 0).all()
        want = ft.add_deltas_host(ft.kaldi_fbank_host(waves[k], CFG, np.float32), 2)
        assert np.array_equal(a['features'][r, :frames[k]].numpy(), want)


def test_supported_and_argument_checks_need_no_gpu():
    L = _native.lib()
    assert L.asr_abi_version() == 24
    assert L.asr_fbank_supported(400, 160, 512, 80, 2, 2) == 1
    assert L.asr_fbank_supported(400, 160, 512, 40, 0, 2) == 1
    assert L.asr_fbank_supported(512, 1, 512, 128, 1, 2) == 1
    for bad in ((400, 160, 1024, 80, 2, 2), (256, 160, 512, 80, 2, 2), (513, 160, 512, 80, 2, 2),
                (400, 160, 512, 0, 2, 2), (400, 160, 512, 129, 2, 2), (400, 160, 512, 80, 3, 2),
                (400, 160, 512, 80, -1, 2), (400, 160, 512, 80, 2, 3), (400, 0, 512, 80, 2, 2)):
        assert L.asr_fbank_supported(*bad) == 0, bad
    assert ft.native_supported(CFG) and not ft.native_supported(ft.make_config(frame_length=200))

    one = 0x1000                # never dereferenced: every call below is answered before a launch

    def call(waves=one, lens=one, B=1, T_max=1, tables=one, padded=512, order=2, out=one, stride=400, n_max=400):
        return L.asr_fbank_f32(waves, stride, n_max, 1, lens, B, T_max, tables, tables, tables, tables, 501,
                               400, 160, padded, 80, 1, order, 2, 0.97, None, None, 0.0, 0, 0, out, out, None)
    assert call(waves=None) == _native.ASR_EINVAL
    assert call(lens=None) == _native.ASR_EINVAL
    assert call(tables=None) == _native.ASR_EINVAL
    assert call(out=None) == _native.ASR_EINVAL
    assert call(B=-1) == _native.ASR_EINVAL
    assert call(T_max=0) == _native.ASR_EINVAL
    assert call(stride=399) == _native.ASR_EINVAL
    assert call(padded=1024) == _native.ASR_EUNSUPPORTED
    assert call(order=3) == _native.ASR_EUNSUPPORTED
    assert call(B=0) == _native.ASR_OK


def test_extract_features_tool(tmp_path):
    import importlib.util
    import os
    import wave
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('extract_features', os.path.join(ROOT, 'tools', 'extract_features.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    utts = [_wave(400 + 160 * 3 + 11, seed=21), _wave(400 + 160 * 7, seed=22)]
    paths = []
    for k, u in enumerate(utts):
        paths.append(str(tmp_path / ('u%d.wav' % k)))
        with wave.open(paths[-1], 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(u.astype('<i2').tobytes())
    out = str(tmp_path / 'feats.npz')
    tool.main(paths + ['--out', out, '--cpu', '--num-mel-bins', '40', '--delta-order', '1'])
    got = np.load(out)
    assert list(got['order']) == [1, 0] and list(got['features_lengths']) == [8, 4]
    assert got['features'].shape == (2, 8, 41, 2)
    cfg = ft.make_config(num_mel_bins=40, delta_order=1)
    want = ft.add_deltas_host(ft.kaldi_fbank_host(utts[0], cfg, np.float32), 1)
    assert np.array_equal(got['features'][1, :4], want) and not got['features'][1, 4:].any()
