"""The feature front-end on the MI355X (csrc/fbank.hip through att_speech.features.KaldiFbank)
against the numpy twin in fp64.  Inputs, twins and the measured tolerance: tests/fbank_cases.py
(per channel, the device may miss the fp64 twin by 4 times what the fp32 twin misses it by)."""
import numpy as np
import pytest
import torch

import fbank_cases as fc
from att_speech import features as ft

pytestmark = pytest.mark.gpu

LOG_EPS = float(np.log(np.float64(ft.FLT_EPSILON)))


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def run(c, wave_dtype=torch.int16, **kw):
    waves = torch.from_numpy(c.waves).to(dev()).to(wave_dtype)
    return c.fe(waves, c.wave_lens, **kw)


def check_accuracy(c, out, what):
    assert c.gap32_static <= fc.GAP32_STATIC_MAX, (what, c.gap32_static)
    err = fc.errors(out['features'].cpu().numpy(), c)
    print('%s: err %s gap32 %s ratio %s' % (what, err, c.gap32, err / c.gap32))
    assert (err <= fc.FACTOR * c.gap32).all(), (what, err, c.gap32, err / c.gap32)


@pytest.mark.parametrize('wave_dtype', [torch.int16, torch.float32], ids=['int16', 'fp32'])
@pytest.mark.parametrize('family', fc.FAMILIES)
@pytest.mark.parametrize('config', list(fc.CONFIGS))
def test_device_matches_fp64_twin(config, family, wave_dtype):
    c = fc.case(config, family)
    out = run(c, wave_dtype)
    F, C = c.fe.feat_dim, c.fe.channels
    assert out['features'].shape == (len(c.frames), c.T_max, F, C)
    assert out['features'].dtype == torch.float32 and out['features'].is_contiguous()
    assert out['features'].device.type == 'cuda'
    check_accuracy(c, out, '%s/%s/%s' % (config, family, wave_dtype))


def test_lengths_and_padding_frames_are_exact():
    c = fc.case('recipe', 'noise')
    waves = torch.from_numpy(c.waves).to(dev())
    out = c.fe(waves, c.wave_lens)
    lens = out['features_lengths']
    assert lens.dtype == torch.int32 and not lens.is_cuda
    assert lens.tolist() == [1 + (n - 400) // 160 for n in c.wave_lens] == c.frames
    from att_speech import _native
    assert _native.lens_on(lens, dev()).tolist() == c.frames        # the kernel's own count, attached
    # pre-filled with NaN, a larger T_max: every padding entry is written, and written 0
    T_max = c.T_max + 37
    buf = torch.full((len(c.frames), T_max, c.fe.feat_dim, c.fe.channels), float('nan'), device=dev())
    got, dev_lens = c.fe._native(waves, c.wave_lens, T_max, 0, 0, out=buf)
    assert got.data_ptr() == buf.data_ptr() and dev_lens.tolist() == c.frames
    for b, T in enumerate(c.frames):
        assert (got[b, T:] == 0).all()
        assert torch.isfinite(got[b, :T]).all()
        assert torch.equal(got[b, :T], out['features'][b, :T])


def test_all_zero_utterance():
    fe = ft.KaldiFbank()
    waves = torch.zeros(2, 400 + 160 * 36 + 5, dtype=torch.int16, device=dev())
    out = fe(waves, [waves.size(1), 400])['features'].cpu().numpy()
    for b, T in ((0, 37), (1, 1)):
        assert np.abs(out[b, :T, :, 0] - LOG_EPS).max() <= 2e-6
        assert np.abs(out[b, :T, :, 1:]).max() <= 4e-6
        assert (out[b, T:] == 0).all()


def test_rows_do_not_depend_on_the_batch():
    c = fc.case('recipe', 'speech')
    waves = torch.from_numpy(c.waves).to(dev())
    full = c.fe(waves, c.wave_lens)['features']
    again = c.fe(waves, c.wave_lens)['features']
    assert torch.equal(full, again)
    flipped = c.fe(waves.flip(0).contiguous(), c.wave_lens[::-1], t_max=c.T_max + 50)['features']
    for b in (0, 4, 7, 9, 13):
        T, n = c.frames[b], c.wave_lens[b]
        alone = c.fe(waves[b:b + 1, :n].contiguous(), [n])['features']
        assert alone.shape[1] == T
        assert torch.equal(alone[0], full[b, :T])
        assert torch.equal(flipped[len(c.frames) - 1 - b, :T], full[b, :T])
        assert (flipped[len(c.frames) - 1 - b, T:] == 0).all()


def test_dither():
    c = fc.case('recipe', 'noise', 1.0, 3, 5)
    out = run(c, seed=3, iteration=5)
    check_accuracy(c, out, 'dither')
    assert torch.equal(run(c, seed=3, iteration=5)['features'], out['features'])
    other = run(c, seed=3, iteration=6)['features']
    plain = run(fc.case('recipe', 'noise'))['features']
    valid = torch.zeros(out['features'].shape[:2], dtype=torch.bool)
    for b, T in enumerate(c.frames):
        valid[b, :T] = True
    valid = valid.to(dev())
    # every frame draws afresh: no frame keeps its features under another iteration or without dither
    assert (other != out['features']).flatten(2).any(dim=2)[valid].all()
    assert (plain != out['features']).flatten(2).any(dim=2)[valid].all()


def test_host_paths_return_the_twin(monkeypatch):
    c = fc.case('recipe', 'speech')
    want = torch.from_numpy(c.twin32)
    cpu = c.fe(torch.from_numpy(c.waves), c.wave_lens)
    assert not cpu['features'].is_cuda and torch.equal(cpu['features'], want)
    monkeypatch.setenv('ASR_FBANK_NATIVE', '0')
    off = run(c)
    assert off['features'].is_cuda and torch.equal(off['features'].cpu(), want)
    monkeypatch.delenv('ASR_FBANK_NATIVE')
    assert not torch.equal(run(c)['features'].cpu(), want)       # the kernel's own rounding


def test_features_feed_the_wsj_model():
    from att_speech.models import SpeechModel
    from att_speech.modules.encoders import native_conv
    from test_modules import DEC_MONO, ENC, VOCAB, sample_batch
    torch.manual_seed(3)
    utts = fc.utterances('speech')[-5:]
    waves, wave_lens, order = ft.collate_waves(utts)
    fe = ft.KaldiFbank()
    out = fe(torch.from_numpy(waves).to(dev()), wave_lens)
    feats, lens = out['features'], out['features_lengths']
    assert feats.shape == (5, 100, 81, 3) and lens.tolist() == [100, 65, 64, 63, 33]
    assert feats.float().contiguous().data_ptr() == feats.data_ptr()         # conv1 takes it as it is
    model = SpeechModel(dict(ENC, rnn_nb_layers=1), DEC_MONO, sample_batch(B=2, T=100, F=81, ch=3), 49, VOCAB)
    model.to(dev()).eval()
    assert native_conv.first_supported(model.encoder.conv[0], feats.permute(0, 3, 1, 2))
    with torch.no_grad():
        enc, enc_lens = model.encoder(feats, lens, None)
    assert enc.size(1) == 5 and int(enc_lens[0]) == enc.size(0)
    assert torch.isfinite(enc.float()).all()
