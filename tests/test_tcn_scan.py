"""The TCN decoder's native training scan (asr_tcn_attention_scan_*_f32, ABI v24) without a
GPU: the C ABI exports both entry points and refuses bad arguments before launching, and
the decoder's gate keeps the per-position loop wherever the scan does not apply."""
import warnings

import pytest
import torch

warnings.filterwarnings('ignore')


def _lib():
    from att_speech import _native
    return _native, _native.lib()


def test_scan_symbols_exported_at_abi_24():
    _native, L = _lib()
    assert _native.ABI_VERSION == 24 and L.asr_abi_version() == 24
    assert hasattr(L, 'asr_tcn_attention_scan_fwd_f32')
    assert hasattr(L, 'asr_tcn_attention_scan_bwd_f32')


def _fwd(L, ptr, T=10, B=2, Lq=3, A=8, K=32, last=None):
    return L.asr_tcn_attention_scan_fwd_f32(ptr, ptr, ptr, ptr, ptr, ptr, 1.25, ptr,
                                            T, B, Lq, A, K, ptr if last is None else last, None)


def _bwd(L, ptr, T=10, B=2, Lq=3, A=8, K=32, last=None):
    return L.asr_tcn_attention_scan_bwd_f32(ptr, ptr, ptr, ptr, ptr, 1.25, ptr, ptr, ptr,
                                            T, B, Lq, A, K, ptr, ptr, ptr, ptr,
                                            ptr if last is None else last, None)


@pytest.mark.parametrize('call', [_fwd, _bwd])
def test_scan_argument_checks_need_no_gpu(call):
    _native, L = _lib()
    # a non-null dummy address: every check below must fire before anything is launched
    p = 0x1000
    assert call(L, None) == _native.ASR_EINVAL                  # null pointers
    assert call(L, p, T=0) == _native.ASR_EINVAL
    assert call(L, p, B=0) == _native.ASR_EINVAL
    assert call(L, p, Lq=0) == _native.ASR_EINVAL
    assert call(L, p, A=0) == _native.ASR_EINVAL
    assert call(L, p, T=-3) == _native.ASR_EINVAL
    assert call(L, p, K=3) == _native.ASR_EUNSUPPORTED          # only the 32-tap filter
    assert call(L, p, A=257) == _native.ASR_EUNSUPPORTED
    assert call(L, p, T=4097) == _native.ASR_EUNSUPPORTED
    # one null output among valid shapes
    assert call(L, p, last=0) == _native.ASR_EINVAL


def _decoder(**kw):
    from att_speech.modules.tcn import AttentionDecoderTCN
    args = dict(tcn_hidden_size=24, att_hidden_size=8, dropout_p=0.0, kernel_size=3,
                dilation_sizes=[1, 2], attention_temperature=1.25)
    args.update(kw)
    return AttentionDecoderTCN({'features': torch.zeros(5, 2, 16)}, 7, **args)


class _FakeCuda(object):
    """Stands in for a CUDA tensor in the gate (shape, dtype, is_cuda only)."""

    def __init__(self, T, dtype=torch.float32):
        self.is_cuda, self.dtype, self._T = True, dtype, T

    def size(self, d):
        return (self._T, 2, 16)[d]


def test_native_train_gate(monkeypatch):
    monkeypatch.delenv('ASR_TCN_TRAIN_NATIVE', raising=False)
    dec = _decoder()
    assert not dec._native_train_ok(torch.zeros(5, 2, 16))             # CPU tensor
    assert dec._native_train_ok(_FakeCuda(5))
    assert not dec._native_train_ok(_FakeCuda(5, torch.float64))
    assert dec._native_train_ok(_FakeCuda(4096))
    assert not dec._native_train_ok(_FakeCuda(4097))                   # the kernels' limit
    monkeypatch.setenv('ASR_TCN_TRAIN_NATIVE', '0')                    # read per call
    assert not dec._native_train_ok(_FakeCuda(5))
    monkeypatch.setenv('ASR_TCN_TRAIN_NATIVE', '1')
    assert dec._native_train_ok(_FakeCuda(5))
    assert not _decoder(att_force_forward=(-2, 8))._native_train_ok(_FakeCuda(5))
    assert not _decoder(att_hidden_size=257)._native_train_ok(_FakeCuda(5))


def test_cpu_forward_is_the_loop(monkeypatch):
    """On the CPU the gate is closed whatever the switch says: the loop's numbers stay."""
    torch.manual_seed(3)
    dec = _decoder()
    enc = torch.randn(9, 2, 16)
    texts = torch.tensor([[2, 3, 4], [5, 0, 0]])
    outs = []
    for flag in ('1', '0'):
        monkeypatch.setenv('ASR_TCN_TRAIN_NATIVE', flag)
        outs.append(dec(enc, torch.tensor([9, 6]), texts, torch.tensor([3, 1]),
                        return_att_weights=True))
    assert torch.equal(outs[0]['loss'], outs[1]['loss'])
    assert len(outs[0]['attweights']) == 4
