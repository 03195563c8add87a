"""Native BiGRU recurrence (csrc/gru.hip, bf16 MFMA operands / fp32 state) against torch's fp32
nn.GRU on a packed batch on the CPU, the persistent kernels against the per-step ones bit for
bit, and the GRU encoder through SpeechModel / dp.train_step."""
import copy
import os

import numpy as np
import pytest
import torch
from torch import nn

from test_gru_abi import emulate_gru_bf16_operands
from test_modules import DEC_MONO, ENC, VOCAB, sample_batch

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ragged(T, B, seed):
    lens = sorted(np.random.RandomState(seed).randint(1, T + 1, size=B).tolist(), reverse=True)
    lens[0] = T
    return torch.tensor(lens)


@pytest.mark.parametrize('T,B,F,H', [(37, 5, 48, 64), (40, 24, 352, 320), (25, 33, 320, 320)])
def test_bigru_is_the_bf16_operand_evaluation(T, B, F, H):
    from att_speech.modules.encoders.native_gru import bigru
    torch.manual_seed(T * 77 + B)
    lens_t = _ragged(T, B, B + 1)
    rnn = nn.GRU(F, H, bidirectional=True, bias=False)
    x = torch.randn(T, B, F)
    with torch.no_grad():
        emu = emulate_gru_bf16_operands(x, lens_t, rnn)
        packed = nn.utils.rnn.pack_padded_sequence(x, lens_t)
        y32, _ = nn.utils.rnn.pad_packed_sequence(rnn(packed)[0], total_length=T)
    rnn_g = copy.deepcopy(rnn).to(dev())
    with torch.no_grad():
        y = bigru(x.to(dev()), lens_t, rnn_g).view(T, B, 2 * H).cpu()
    scale = float(y32.abs().max())
    to_emu = float((y - emu).abs().max())
    emu_to_32 = float((emu - y32).abs().max())
    gpu_to_32 = float((y - y32).abs().max())
    assert to_emu <= 2e-3 * scale, (to_emu, scale)
    assert float((y - emu).abs().mean()) <= 5e-5 * scale
    assert gpu_to_32 <= 1.5 * emu_to_32 + 2e-3 * scale, (gpu_to_32, emu_to_32)


def _ref(x, lens, rnn, dy):
    x = x.clone().requires_grad_()
    packed = nn.utils.rnn.pack_padded_sequence(x, lens)
    y, _ = rnn(packed)
    y, _ = nn.utils.rnn.pad_packed_sequence(y, total_length=x.size(0))
    y.backward(dy)
    return y.detach(), x.grad, [p.grad.clone() for p in rnn.parameters()]


@pytest.mark.parametrize('T,B,F,H,lens', [
    (37, 5, 48, 64, [37, 30, 30, 11, 1]),
    (60, 40, 352, 320, None),
    (12, 33, 320, 320, None),
    (21, 9, 128, 128, None),
    (15, 6, 256, 256, None),
])
@pytest.mark.parametrize('sum_dirs', [False, True])
def test_bigru_matches_packed_torch_gru(T, B, F, H, lens, sum_dirs):
    from att_speech.modules.encoders.native_gru import bigru
    torch.manual_seed(T * 1000 + B)
    lens_t = torch.tensor(lens) if lens is not None else _ragged(T, B, B)
    rnn = nn.GRU(F, H, bidirectional=True, bias=False)
    x = torch.randn(T, B, F)
    mask = (torch.arange(T)[:, None] < lens_t[None, :]).float()[:, :, None]
    dy = torch.randn(T, B, 2 * H) * mask
    if sum_dirs:
        g = dy.view(T, B, 2, H)[:, :, 0].contiguous()
        dy = torch.stack([g, g], 2).view(T, B, 2 * H)
    y_ref, dx_ref, dw_ref = _ref(x, lens_t, rnn, dy)
    rnn_g = copy.deepcopy(rnn).to(dev())
    rnn_g.zero_grad()
    xg = x.to(dev()).requires_grad_()
    if sum_dirs:
        y = bigru(xg, lens_t, rnn_g, sum_dirs=True)
        assert tuple(y.shape) == (T, B, H)
        y.backward(g.to(dev()))
        y_ref = y_ref.view(T, B, 2, H).sum(2)
        pad = (mask.expand(T, B, H) == 0)
    else:
        y = bigru(xg, lens_t, rnn_g).view(T, B, 2 * H)
        y.backward(dy.to(dev()))
        pad = (mask.expand(T, B, 2 * H) == 0)

    def close(a, b, what, rtol):
        a, b = a.detach().cpu(), b.detach().cpu()
        err = float((a - b).abs().max())
        scale = float(b.abs().max()) + 1e-6
        assert err <= rtol * scale, (what, err, scale)

    close(y, y_ref, 'y', 3e-2)
    assert not y.detach().cpu()[pad].any()                      # zeros on padding
    assert not xg.grad.cpu()[mask.expand(T, B, F) == 0].any()   # no gradient reaches padding
    close(xg.grad, dx_ref, 'dx', 5e-2)
    for p, w in zip(rnn_g.parameters(), dw_ref):
        close(p.grad, w, 'dw', 5e-2)


def _run_native(gx, whh, lens, dy, persist):
    from att_speech import _native
    os.environ['ASR_LSTM_PERSIST'] = '1' if persist else '0'
    try:
        y, ybf, gates = _native.gru_bidir_fwd(gx, whh, lens)
        whhT = whh.transpose(1, 2).contiguous()
        dgx, dhn = _native.gru_bidir_bwd(dy, whhT, lens, gates, y)
        torch.cuda.synchronize()
    finally:
        os.environ.pop('ASR_LSTM_PERSIST', None)
    _native.lstm_check_errors()
    return y, ybf, gates, dgx, dhn


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize('T,B,H,reps', [
    (1, 1, 64, 1),             # a single frame, a single utterance
    (2, 3, 64, 1),
    (23, 7, 64, 1),            # one workgroup per team, ragged batch tile
    (61, 45, 128, 1),          # two-workgroup teams
    (19, 70, 256, 1),
    (150, 96, 320, 1),         # five-workgroup teams (the recipes' hidden size)
    (334, 768, 320, 3),        # bench shape, repeated
    (40, 900, 320, 1),         # more batch tiles than one resident launch holds
])
def test_persistent_recurrence_is_bitwise_the_per_step_one(T, B, H, reps):
    from att_speech import _native
    assert _native.gru_supported(B, H)
    g = torch.Generator().manual_seed(T * 31 + B)
    lens = torch.randint(1, T + 1, (B,), generator=g).sort(descending=True)[0]
    lens[0] = T
    gx = (torch.randn(T, B, 2, 3 * H, generator=g) * 1.5).to(dev())
    whh = (torch.randn(2, 3 * H, H, generator=g) * (1.0 / H ** 0.5)).to(dev(), torch.bfloat16)
    dy = torch.randn(T, B, 2, H, generator=g).to(dev())
    lens_d = lens.to(dev(), torch.int32)
    runs = [gx] * reps + ([gx.to(torch.bfloat16)] if reps == 1 else [])    # fp32 and bf16 x.W_ih
    ref_cache = {}
    for gxi in runs:
        if gxi.dtype not in ref_cache:
            ref_cache[gxi.dtype] = _run_native(gxi, whh, lens_d, dy, persist=False)
        ref = ref_cache[gxi.dtype]
        out = _run_native(gxi, whh, lens_d, dy, persist=True)
        for name, a, b in zip(('y', 'y_bf16', 'gates', 'dgx', 'dhn'), out, ref):
            assert not torch.isnan(a.float()).any(), name
            assert torch.equal(_bits(a), _bits(b)), (name, float((a.float() - b.float()).abs().max()))
    # the shared gradient form (dy [T,B,H]) too
    dys = dy[:, :, 0].contiguous()
    outs = []
    for persist in (False, True):
        os.environ['ASR_LSTM_PERSIST'] = '1' if persist else '0'
        try:
            y, _, gates = _native.gru_bidir_fwd(gx, whh, lens_d)
            outs.append(_native.gru_bidir_bwd(dys, whh.transpose(1, 2).contiguous(), lens_d, gates, y))
        finally:
            os.environ.pop('ASR_LSTM_PERSIST', None)
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))


def test_padding_garbage_reaches_no_output():
    """Large finite values in the padded frames of x leave every output and gradient bitwise
    unchanged (the input projection of padding frames lands in gx rows the recurrence must
    never read into a result)."""
    from att_speech.modules.encoders.native_gru import bigru
    torch.manual_seed(9)
    T, B, F, H = 30, 20, 96, 320
    lens = _ragged(T, B, 5)
    rnn = nn.GRU(F, H, bidirectional=True, bias=False).to(dev())
    x = torch.randn(T, B, F, device=dev())
    pad = (torch.arange(T)[:, None] >= lens[None, :]).to(dev())
    x2 = x.clone()
    x2[pad] = 3e4 * torch.sign(torch.randn_like(x2[pad]))
    dy = torch.randn(T, B, H, device=dev())
    res = []
    for xi in (x, x2):
        rnn.zero_grad()
        xi = xi.clone().requires_grad_()
        y = bigru(xi, lens, rnn, sum_dirs=True)
        y.backward(dy)
        res.append([y.detach(), xi.grad[~pad]] + [p.grad.clone() for p in rnn.parameters()])
    for a, b in zip(*res):
        assert torch.isfinite(a).all()
        assert torch.equal(_bits(a), _bits(b))


def test_handoff_timeout_surfaces_as_an_error(monkeypatch):
    """The bounded spin's give-up path, forced with the debug bound ASR_LSTM_SPIN_LIMIT=0 (a
    software timeout): the GRU sets the same error word as the LSTM, its outputs are NaN,
    lstm_check_errors raises, and the next call is clean."""
    from att_speech import _native
    from att_speech.modules.encoders.native_gru import bigru
    torch.manual_seed(0)
    T, B, F, H = 6, 40, 64, 320          # five workgroups per team -> real hand-offs
    rnn = nn.GRU(F, H, bidirectional=True, bias=False).to(dev())
    x = torch.randn(T, B, F, device=dev())
    lens = torch.full((B,), T, dtype=torch.int64)
    _native.lstm_check_errors()
    monkeypatch.setenv('ASR_LSTM_SPIN_LIMIT', '0')
    y = bigru(x, lens, rnn)
    torch.cuda.synchronize()
    assert int(_native.lstm_error_word(x.device).item()) != 0
    with pytest.raises(RuntimeError, match='hand-off timed out'):
        _native.lstm_check_errors()
    assert not bool(torch.isfinite(y).all())
    monkeypatch.delenv('ASR_LSTM_SPIN_LIMIT')
    y = bigru(x, lens, rnn)
    _native.lstm_check_errors()
    assert bool(torch.isfinite(y).all())


ENC_GRU = dict(ENC, rnn_type='GRU')


def _count_calls(monkeypatch):
    from att_speech import _native
    calls = {'fwd': 0, 'bwd': 0}
    real_f, real_b = _native.gru_bidir_fwd, _native.gru_bidir_bwd

    def f(*a, **k):
        calls['fwd'] += 1
        return real_f(*a, **k)

    def b(*a, **k):
        calls['bwd'] += 1
        return real_b(*a, **k)
    monkeypatch.setattr(_native, 'gru_bidir_fwd', f)
    monkeypatch.setattr(_native, 'gru_bidir_bwd', b)
    return calls


@pytest.mark.parametrize('F,ch', [(40, 1), (81, 3)])
def test_gru_speech_model_train_step_matches_cpu(oracle_lib, monkeypatch, F, ch):
    import warnings
    from att_speech.models import SpeechModel
    from test_model_gpu import cpu_reference_loss, make_batch
    torch.manual_seed(7)
    B, T, L, S = 4, 150, 10, 49
    feats, lens, texts, llens = make_batch(B, T, S, L, 1, 11, F, ch)
    model = SpeechModel(ENC_GRU, DEC_MONO, sample_batch(B=2, T=T, F=F, ch=ch), S, VOCAB)
    assert all(isinstance(m.rnn, nn.GRU) for m in model.encoder.rnns)
    model.train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.eval()
    ref = copy.deepcopy(model)
    want, want_g = cpu_reference_loss(ref, feats, lens, texts, llens, oracle_lib, 1, denominator=False)
    calls = _count_calls(monkeypatch)
    model.to(dev())
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        warnings.filterwarnings('ignore', message='^(?!.*no hand-written recurrence)')
        out = model(feats.to(dev()), lens, None, texts, llens)
        out['loss'].backward()
    n = len(model.encoder.rnns)
    assert calls == {'fwd': n, 'bwd': n}, calls
    got = float(out['loss'])
    assert abs(got - want) <= 2e-2 * abs(want), (got, want)
    for k, p in model.named_parameters():
        g, w = p.grad.cpu().flatten(), want_g[k].flatten()
        if float(w.norm()) > 1e-4:
            cos = float(torch.dot(g, w) / (g.norm() * w.norm() + 1e-20))
            assert cos > 0.98, (k, cos)


def test_gru_train_step_with_fused_adam_is_deterministic(monkeypatch):
    """One dp.train_step with FusedClipAdam on the GRU model: two identical runs give bitwise
    identical parameters, and the step reads the recurrence's error word."""
    from att_speech import _native
    from att_speech.dp import FlatGradBucket, train_step
    from att_speech.fused_step import FusedClipAdam
    from att_speech.models import SpeechModel
    from att_speech.modules.hooks import GradientClipping
    from test_model_gpu import make_batch
    torch.manual_seed(7)
    B, T, L, S = 4, 150, 10, 49
    feats, lens, texts, llens = make_batch(B, T, S, L, 1, 11)
    m0 = SpeechModel(ENC_GRU, DEC_MONO, sample_batch(B=2, T=T), S, VOCAB)
    words = []
    real_word = _native.lstm_error_word

    def word(device):
        w = real_word(device)
        words.append(w)
        return w
    monkeypatch.setattr(_native, 'lstm_error_word', word)
    runs = []
    for _ in range(2):
        model = copy.deepcopy(m0).to(dev())
        bucket = FlatGradBucket(model.parameters())
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        hooks = [GradientClipping(clip_norm=30.0, skip_step_norm=1e6)]
        for h in hooks:
            h.pre_run(model, opt)
        fused = FusedClipAdam.from_optimizer(opt, bucket, hooks[0])
        out, skip = train_step(model, opt, ((feats.to(dev()), lens, None, texts, llens), {}),
                               hooks=hooks, bucket=bucket, fused=fused)
        assert not skip and np.isfinite(float(out['loss']))
        fused.drain()
        runs.append([p.detach().clone() for p in model.parameters()])
    assert words and all(w is not None for w in words)        # the GRU's error word was read
    assert int(words[-1].item()) == 0
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


def test_lstm_speech_model_still_takes_the_stack(monkeypatch):
    """An LSTM encoder still runs as one bilstm_stack node (the GRU branch keeps
    _plain_native_stack LSTM-only), and a GRU encoder never reaches it."""
    from att_speech.models import SpeechModel
    from att_speech.modules.encoders import native_lstm
    calls = {'stack': 0}
    real = native_lstm.bilstm_stack

    def stack(*a, **k):
        calls['stack'] += 1
        return real(*a, **k)
    monkeypatch.setattr(native_lstm, 'bilstm_stack', stack)
    from test_model_gpu import make_batch
    torch.manual_seed(3)
    B, T = 2, 100
    feats, lens = make_batch(B, T, 49, 10, 1, 11)[:2]
    for enc, want in ((ENC, 1), (ENC_GRU, 0)):
        calls['stack'] = 0
        model = SpeechModel(enc, DEC_MONO, sample_batch(B=B, T=T), 49, VOCAB).to(dev())
        with torch.no_grad():
            y, _ = model.encoder(feats.to(dev()), lens, None)
        assert calls['stack'] == want, (enc.get('rnn_type'), calls)
        assert torch.isfinite(y).all()
