"""att_speech.modules.decoders.attention_decoder (Attention, AttentionDecoderRNN) without a GPU:
the class resolves at the reference's dotted path, carries the reference's checkpoint keys,
and its torch-op path reproduces what the reference's own class computed on the seeded inputs
of tests/golden/attention_rnn.npz (made by tests/golden/make_golden_attention_rnn.py): loss,
alignments, states, every gradient, decoded labels and scores.  Both sides are fp32 torch on a
CPU (the reference's own fp32-vs-fp64 distance on such inputs is 1e-7), so everything is held
to 1e-5 of each tensor's largest magnitude.  The C ABI exports the two scan entry points and
refuses bad arguments before launching; the gate keeps the loop wherever the scan does not
apply."""
import re
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import golden

warnings.filterwarnings('ignore')

PATH = 'att_speech.modules.decoders.attention_decoder.AttentionDecoderRNN'
SWITCH = 'ASR_ATT_RNN_NATIVE'
RTOL = 1e-5


def get_class():
    from att_speech import utils
    return utils.get_class(PATH)


def build(g, prefix='', **kw):
    """the decoder of one fixture record with the record's weights loaded"""
    T, B, E = g['enc'].shape
    sd = {k[len(prefix) + 3:]: torch.from_numpy(g[k]) for k in g.files
          if k.startswith(prefix + 'sd_')}
    args = dict(n_layers=sd['rnn_zero_state'].shape[0], hidden_size=sd['rnn_zero_state'].shape[2],
                dropout_p=0.0, beam_size=3, length_normalization=float(g['length_normalization']))
    args.update(kw)
    dec = get_class()({'features': torch.zeros(T, B, E)}, int(g['S']), **args)
    dec.load_state_dict(sd, strict=True)
    return dec, sd


def batch(g):
    return (torch.from_numpy(g['enc']), torch.from_numpy(g['lens']),
            torch.from_numpy(g['texts']), torch.from_numpy(g['text_lens']))


def close(name, got, want, rtol=RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    assert err <= rtol * scale, (name, err / scale)


def check_forward(g, prefix, dec, enc, lens, texts, tl):
    out = dec(enc, lens, texts, tl, return_att_weights=True, return_rnn_states=True)
    close(prefix + 'loss', out['loss'].detach(), g[prefix + 'loss'])
    assert isinstance(out['attweights'], list) and isinstance(out['rnnstates'], list)
    close(prefix + 'att', torch.stack(out['attweights']).detach(), g[prefix + 'att'])
    close(prefix + 'states', torch.stack(out['rnnstates']), g[prefix + 'states'])
    assert not out['rnnstates'][0].requires_grad
    return out


def test_class_resolves_at_the_reference_path():
    from att_speech.modules.decoders import attention_decoder
    cls = get_class()
    assert cls is attention_decoder.AttentionDecoderRNN
    assert issubclass(attention_decoder.Attention, torch.nn.Module)


def test_state_dict_keys_and_shapes():
    g = golden('attention_rnn.npz')
    for prefix in ('', 'l2_'):
        dec, sd = build(g, prefix)
        own = dec.state_dict()
        assert list(own.keys()) == list(sd.keys())
        assert {k: tuple(v.shape) for k, v in own.items()} == \
            {k: tuple(v.shape) for k, v in sd.items()}
    fresh = get_class()({'features': torch.zeros(4, 2, 16)}, 7, n_layers=1, hidden_size=24,
                        dropout_p=0.3)
    assert float(fresh.attn.hidden_to_score.weight.detach().abs().max()) == 0.0
    assert fresh.num_classes == 8 and fresh.EOS == 7 and fresh.TRANSCRIPTION_LEN_GUARD == 400
    assert isinstance(fresh.dropout, torch.nn.Dropout) and fresh.rnn.bias
    assert fresh.rnn.input_size == 24 + 16 and fresh.attn.hidden_size == 24
    assert tuple(fresh.rnn_zero_state.shape) == (1, 1, 24)


def test_forward_and_gradients_match_the_reference():
    g = golden('attention_rnn.npz')
    dec, sd = build(g)
    enc, lens, texts, tl = batch(g)
    x = enc.clone().requires_grad_()
    before = texts.clone()
    out = check_forward(g, '', dec, x, lens, texts, tl)
    assert torch.equal(texts, before)
    assert len(out['attweights']) == texts.size(1) + 1
    assert tuple(out['attweights'][0].shape) == (enc.size(0), enc.size(1))
    out['loss'].backward()
    for name, prm in dec.named_parameters():
        close('grad_' + name, prm.grad, g['grad_' + name])
    close('grad_encoded', x.grad, g['grad_encoded'])


def test_init_attention_and_padding():
    g = golden('attention_rnn.npz')
    dec, _ = build(g)
    enc, lens, texts, tl = batch(g)
    (eproj, pad), first = dec.attn.init_attention(enc, lens)
    assert tuple(eproj.shape) == (enc.size(0), enc.size(1), dec.hidden_size)
    assert torch.equal(first[0], torch.ones(enc.size(1))) and float(first[1:].abs().max()) == 0
    for b, n in enumerate(lens.tolist()):
        assert float(pad[:n, b].abs().max()) == 0 and bool((pad[n:, b] == -1e5).all())
    att = torch.stack(dec(enc, lens, texts, tl, return_att_weights=True)['attweights'])
    for b, n in enumerate(lens.tolist()):
        assert not bool((att[:, n:, b] != 0).any())
    np.testing.assert_allclose(att.sum(1).detach().numpy(), 1.0, atol=3e-6)


def test_force_forward_record():
    g = golden('attention_rnn.npz')
    dec, _ = build(g, 'ff_', att_force_forward=tuple(int(v) for v in g['ff_window']))
    check_forward(g, 'ff_', dec, *batch(g))
    # the window bites: the same weights without it give other alignments
    plain, _ = build(g, 'ff_')
    att = torch.stack(plain(*batch(g), return_att_weights=True)['attweights']).detach().numpy()
    assert np.abs(att - g['ff_att']).max() > 1e-3


def test_two_layer_record():
    g = golden('attention_rnn.npz')
    dec, _ = build(g, 'l2_')
    assert dec.n_layers == 2
    out = check_forward(g, 'l2_', dec, *batch(g))
    assert tuple(out['rnnstates'][0].shape) == (2, g['enc'].shape[1], dec.hidden_size)


@pytest.mark.parametrize('beam', [1, 3])
def test_decode_matches_the_reference(beam):
    g = golden('attention_rnn.npz')
    dec, _ = build(g, beam_size=beam)
    dec.eval()
    dec.TRANSCRIPTION_LEN_GUARD = int(g['guard'])
    enc, lens, _, _ = batch(g)
    with torch.no_grad():
        res = dec.decode(enc, lens)
    assert sorted(res) == ['decoded', 'decoded_scores', 'loss']
    key = 'dec%d_' % beam
    got = [[int(c) for c in (d.tolist() if hasattr(d, 'tolist') else d)] for d in res['decoded']]
    assert [len(d) for d in got] == g[key + 'lens'].tolist()
    assert [c for d in got for c in d] == g[key + 'flat'].tolist()
    close(key + 'scores', res['decoded_scores']['acoustic'], g[key + 'scores'])
    close(key + 'loss', res['loss'], g[key + 'loss'])


def test_graph_search_needs_the_hash_the_reference_never_defined():
    from att_speech.lm_fst import LmFst, SymbolTable
    syms = SymbolTable([(0, '<eps>'), (1, '<spc>'), (2, 'a')])
    lm = LmFst(1, 0, [0, 0], [0, 0], [1, 2], [1, 2], [0.5, 0.7], np.array([0.1]), syms, syms)
    dec = get_class()({'features': torch.zeros(4, 1, 8)}, 3, n_layers=1, hidden_size=8,
                      dropout_p=0.0, lm_file=lm, vocabulary=['<pad>', ' ', 'a'],
                      use_graph_search=True)
    assert dec.alphabet_mapping == [1, 1, 2, 1]
    with pytest.raises(AttributeError):
        dec.decode(torch.zeros(4, 1, 8), torch.tensor([4]))


def test_speech_model_trains_one_cpu_step():
    import bench
    from att_speech.models import SpeechModel
    S, B = 49, 2
    feats, lens, texts, llens = bench.synthetic_batch(B, 80, 0, 1)
    texts, llens = texts[:, :6].contiguous(), torch.clamp(llens, max=6)
    for b in range(B):
        texts[b, int(llens[b]):] = 0
    enc_cfg, _ = bench.model_config(1, None)
    dec_cfg = dict(class_name=PATH, n_layers=1, hidden_size=32, dropout_p=0.1, beam_size=1)
    sample = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(), 'spkids': None}
    torch.manual_seed(0)
    model = SpeechModel(enc_cfg, dec_cfg, sample, S, [str(i) for i in range(S)])
    assert type(model.decoder) is get_class()
    opt = torch.optim.Adam(model.get_parameters_for_optimizer(), lr=1e-3)
    loss = model(feats, lens, None, texts, llens)['loss']
    loss.backward()
    assert all(p.grad is not None for p in model.decoder.parameters())
    opt.step()
    assert np.isfinite(float(loss))


# --------------------------------------------------------------------------- the C ABI
NAMES = ('asr_att_gru_scan_fwd_f32', 'asr_att_gru_scan_bwd_f32')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from att_speech import _native
    return _native, _native.lib()


def test_scan_symbols_exported_bound_and_declared():
    _native, L = _lib()
    assert _native.ABI_VERSION == 24 and L.asr_abi_version() == 24
    header = open(os.path.join(ROOT, 'include', 'asr_amd.h')).read()
    for name in NAMES:
        assert hasattr(L, name)
        assert name in _native._SIGNATURES
        assert re.search(r'\bint %s\(' % name, header)
        declared = re.search(r'\bint %s\(([^;]*)\);' % name, header).group(1)
        assert len(declared.split(',')) == len(_native._SIGNATURES[name][1])


def _fwd(L, ptr, T=10, B=6, beam=1, Lq=3, A=8, E=16, H=8, null=None):
    a = [ptr] * 11 + [T, B, beam, Lq, A, E, H] + [ptr] * 5 + [None]
    if null is not None:
        a[null] = None
    return L.asr_att_gru_scan_fwd_f32(*a)


def _bwd(L, ptr, T=10, B=6, beam=1, Lq=3, A=8, E=16, H=8, null=None):
    a = [ptr] * 14 + [T, B, Lq, A, E, H] + [ptr] * 6 + [None]
    if null is not None:
        a[null] = None
    return L.asr_att_gru_scan_bwd_f32(*a)


@pytest.mark.parametrize('call', [_fwd, _bwd])
def test_scan_argument_checks_need_no_gpu(call):
    _native, L = _lib()
    p = 0x1000      # a non-null dummy address: every check must fire before anything is launched
    assert call(L, None) == _native.ASR_EINVAL
    for bad in (dict(T=0), dict(B=0), dict(Lq=0), dict(A=0), dict(E=0), dict(H=0), dict(T=-3)):
        assert call(L, p, **bad) == _native.ASR_EINVAL, bad
    for big in (dict(T=4097), dict(A=324), dict(H=324), dict(E=516), dict(H=10), dict(E=18),
                dict(A=6)):
        assert call(L, p, **big) == _native.ASR_EUNSUPPORTED, big
    assert call(L, p, null=0) == _native.ASR_EINVAL
    assert call(L, p, null=21 if call is _bwd else 18) == _native.ASR_EINVAL      # an output
    # the limits themselves pass the shape check (a null operand stops them before the launch)
    assert call(L, p, T=4096, A=320, E=512, H=320, null=1) == _native.ASR_EINVAL


def test_forward_beam_must_divide_the_hypotheses():
    _native, L = _lib()
    assert _fwd(L, 0x1000, B=6, beam=4) == _native.ASR_EINVAL
    assert _fwd(L, 0x1000, B=6, beam=0) == _native.ASR_EINVAL


# --------------------------------------------------------------------------- the gate
class _FakeCuda(object):
    """Stands in for a CUDA tensor in the gate (shape, dtype, is_cuda only)."""

    def __init__(self, T, dtype=torch.float32, E=16):
        self.is_cuda, self.dtype, self._shape = True, dtype, (T, 2, E)

    def size(self, d):
        return self._shape[d]


def _decoder(E=16, **kw):
    args = dict(n_layers=1, hidden_size=24, dropout_p=0.0)
    args.update(kw)
    return get_class()({'features': torch.zeros(5, 2, E)}, 7, **args)


def test_native_gates(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    dec = _decoder().eval()
    for gate in (dec._native_train_ok, dec._native_decode_ok):
        assert not gate(torch.zeros(5, 2, 16))                     # CPU tensor
        assert gate(_FakeCuda(5))
        assert not gate(_FakeCuda(5, torch.float64))
        assert gate(_FakeCuda(4096))
        assert not gate(_FakeCuda(4097))                           # the kernels' limit
        monkeypatch.setenv(SWITCH, '0')                            # read per call
        assert not gate(_FakeCuda(5))
        monkeypatch.setenv(SWITCH, '1')
        assert gate(_FakeCuda(5))
        monkeypatch.delenv(SWITCH)
    for closed in (_decoder(n_layers=2), _decoder(att_force_forward=(-1, 4)),
                   _decoder(hidden_size=324), _decoder(hidden_size=22), _decoder(E=516)):
        closed.eval()
        fake = _FakeCuda(5, E=closed.encoded_size)
        assert not closed._native_train_ok(fake) and not closed._native_decode_ok(fake)
    for H in (128, 256, 320):
        assert _decoder(E=320, hidden_size=H)._native_train_ok(_FakeCuda(334, E=320))
    assert not _decoder().train()._native_decode_ok(_FakeCuda(5))   # decode: eval mode only
    assert not _decoder(beam_size=33).eval()._native_decode_ok(_FakeCuda(5))


def test_cpu_forward_is_the_loop(monkeypatch):
    """On the CPU the gate is closed whatever the switch says: the loop's numbers stay."""
    g = golden('attention_rnn.npz')
    dec, _ = build(g)
    outs = []
    for flag in ('1', '0'):
        monkeypatch.setenv(SWITCH, flag)
        outs.append(dec(*batch(g), return_att_weights=True))
    assert torch.equal(outs[0]['loss'], outs[1]['loss'])
    assert all(torch.equal(a, b) for a, b in zip(outs[0]['attweights'], outs[1]['attweights']))
