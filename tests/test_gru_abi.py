"""The native GRU recurrence's C ABI (include/asr_amd.h: asr_gru_*) without a GPU: exported,
bound, argument checks before any launch; the CPU BatchRNN(nn.GRU) path unchanged; and the
bf16-operand GRU evaluation that tests/test_gru_gpu.py uses as its arbiter checked against fp32
nn.GRU first."""
import ctypes

import numpy as np
import torch
from torch import nn

GRU_SYMBOLS = ('asr_gru_workspace_bytes', 'asr_gru_supported', 'asr_gru_bidir_fwd_bf16',
               'asr_gru_bidir_bwd_bf16')


def _bf(t):
    return t.to(torch.bfloat16).float()


def emulate_gru_bf16_operands(x, lens, rnn):
    """torch.nn.GRU(bias=False, bidirectional) on a padded batch with the operands of every
    matrix product (x, W_ih, h_{t-1}, W_hh) rounded to bf16, products accumulated in fp32,
    gates and state in fp32: the arithmetic the kernels are built to do."""
    T, B, _ = x.shape
    H = rnn.hidden_size
    out = torch.zeros(T, B, 2, H)
    xb = _bf(x)
    for d, sfx in enumerate(('', '_reverse')):
        wih = _bf(getattr(rnn, 'weight_ih_l0' + sfx).detach())
        whh = _bf(getattr(rnn, 'weight_hh_l0' + sfx).detach())
        for b in range(B):
            L = int(lens[b])
            h = torch.zeros(H)
            for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
                gx = wih @ xb[t, b]
                gh = whh @ _bf(h)
                r = (gx[:H] + gh[:H]).sigmoid()
                z = (gx[H:2 * H] + gh[H:2 * H]).sigmoid()
                n = (gx[2 * H:] + r * gh[2 * H:]).tanh()
                h = (1 - z) * n + z * h
                out[t, b, d] = h
    return out.view(T, B, 2 * H)


def test_gru_symbols_are_exported_and_bound():
    from att_speech import _native
    handle = ctypes.CDLL(_native.LIB_PATH)
    for n in GRU_SYMBOLS:
        assert hasattr(handle, n), n
        assert n in _native._SIGNATURES, n
    L = _native.lib()
    assert L.asr_abi_version() == 24
    assert L.asr_gru_workspace_bytes(768, 320) > 0
    assert L.asr_gru_workspace_bytes(-1, 320) < 0


def test_gru_argument_checks_need_no_gpu():
    from att_speech import _native
    L = _native.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    EINVAL, EUNSUP = _native.ASR_EINVAL, _native.ASR_EUNSUPPORTED
    # null pointers
    assert L.asr_gru_bidir_fwd_bf16(None, 0, p, p, 5, 4, 64, p, p, p, p, big, None, None) == EINVAL
    assert L.asr_gru_bidir_fwd_bf16(p, 0, p, p, 5, 4, 64, None, p, p, p, big, None, None) == EINVAL
    assert L.asr_gru_bidir_bwd_bf16(p, 0, p, p, 5, 4, 64, p, None, p, p, p, big, None, None) == EINVAL
    assert L.asr_gru_bidir_bwd_bf16(p, 0, p, p, 5, 4, 64, p, p, p, None, p, big, None, None) == EINVAL
    # bad shapes / modes / workspace
    assert L.asr_gru_bidir_fwd_bf16(p, 0, p, p, -1, 4, 64, p, p, p, p, big, None, None) == EINVAL
    assert L.asr_gru_bidir_fwd_bf16(p, 0, p, p, 5, 0, 64, p, p, p, p, big, None, None) == EINVAL
    assert L.asr_gru_bidir_fwd_bf16(p, 0, p, p, 5, 4, 70, p, p, p, p, big, None, None) == EINVAL
    assert L.asr_gru_bidir_fwd_bf16(p, 0, p, p, 5, 4, 64, p, p, p, p, 16, None, None) == EINVAL
    assert L.asr_gru_bidir_bwd_bf16(p, 2, p, p, 5, 4, 64, p, p, p, p, p, big, None, None) == EINVAL
    # a hidden size the kernels are not built for
    assert L.asr_gru_bidir_fwd_bf16(p, 0, p, p, 5, 4, 96, p, p, p, p, big, None, None) == EUNSUP
    assert L.asr_gru_bidir_bwd_bf16(p, 0, p, p, 5, 4, 96, p, p, p, p, p, big, None, None) == EUNSUP
    assert L.asr_gru_supported(4, 96) == 0
    assert L.asr_gru_supported(4, 320) & 1


def test_cpu_batchrnn_gru_is_packed_torch_gru():
    from att_speech.modules.encoders.encoder_utils import BatchRNN
    torch.manual_seed(3)
    T, B, F, H = 11, 4, 24, 32
    m = BatchRNN(F, H, rnn_type=nn.GRU, bidirectional=True)
    x = torch.randn(T, B, F)
    lens = torch.tensor([11, 9, 6, 2])
    y, lens_out = m(x, lens)
    packed = nn.utils.rnn.pack_padded_sequence(x, lens)
    want, _ = nn.utils.rnn.pad_packed_sequence(m.rnn(packed)[0], total_length=T)
    assert torch.equal(y, want.view(T, B, 2, H).sum(2))
    assert torch.equal(lens_out, lens)


def test_bf16_operand_emulation_is_within_the_bf16_bound():
    torch.manual_seed(4)
    T, B, F, H = 17, 3, 48, 64
    rnn = nn.GRU(F, H, bidirectional=True, bias=False)
    x = torch.randn(T, B, F)
    lens = torch.tensor([17, 12, 5])
    with torch.no_grad():
        emu = emulate_gru_bf16_operands(x, lens, rnn)
        packed = nn.utils.rnn.pack_padded_sequence(x, lens)
        y32, _ = nn.utils.rnn.pad_packed_sequence(rnn(packed)[0], total_length=T)
    scale = float(y32.abs().max())
    err = float((emu - y32).abs().max())
    # bf16 operands: 8-bit mantissa, a few ulp after the recurrence
    assert err <= 3e-2 * scale, (err, scale)
    assert err > 0          # the emulation does round
    mask = (torch.arange(T)[:, None] < lens[None, :])
    assert not emu[~mask].any()
    assert np.isfinite(emu.numpy()).all()
