"""The TCN decoder's training forward through the native attention scan
(asr_tcn_attention_scan_fwd_f32 / _bwd_f32 behind att_speech.modules.tcn._AttentionScan) on
the MI355X, against the per-position loop it replaces (ASR_TCN_TRAIN_NATIVE=0, same device),
at the lattice_decoding/tcn.yaml dimensions: TCN 384, attention 64, dilations [1, 2], 2 layers
per block, temperature 1.25, 49 symbols + EOS, E = 320.  Where a value misses the loop, an
fp64 evaluation of the loop on the CPU arbitrates."""
import os
import warnings

import numpy as np
import pytest
import torch

warnings.filterwarnings('ignore')

S, E = 49, 320
DEV = torch.device('cuda:0')
SWITCH = 'ASR_TCN_TRAIN_NATIVE'


def make_decoder(A=64, learnable=True, seed=0):
    from att_speech.modules.tcn import AttentionDecoderTCN
    torch.manual_seed(seed)
    dec = AttentionDecoderTCN({'features': torch.zeros(4, 2, E)}, S, tcn_hidden_size=384,
                              att_hidden_size=A, dropout_p=0.0, kernel_size=3,
                              dilation_sizes=[1, 2], tcn_layers_per_block=2,
                              attention_temperature=1.25,
                              learnable_initial_attention=learnable)
    with torch.no_grad():
        for prm in dec.parameters():
            prm.add_(torch.randn_like(prm) * 0.05)
        dec.attn.hidden_to_score.weight.normal_(0.0, 0.5)     # peaky, moving alignments
    return dec


def make_batch(T, lens, text_lens, seed=1):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    enc = torch.randn(T, B, E, generator=g)
    texts = torch.randint(2, S, (B, max(text_lens)), generator=g, dtype=torch.int32)
    for b, n in enumerate(text_lens):
        texts[b, n:] = 0
    return enc, torch.tensor(lens, dtype=torch.int32), texts, torch.tensor(text_lens)


def run(dec, enc, lens, texts, text_lens, native):
    os.environ[SWITCH] = '1' if native else '0'
    try:
        dec.zero_grad(set_to_none=True)
        x = enc.clone().requires_grad_()
        out = dec(x, lens, texts, text_lens, return_att_weights=True)
        out['loss'].backward()
    finally:
        os.environ.pop(SWITCH, None)
    grads = {n: p.grad.detach().clone() for n, p in dec.named_parameters() if p.grad is not None}
    grads['d_encoded'] = x.grad.detach().clone()
    return dict(out=out, loss=out['loss'].detach(), logits=out['logits'].detach(),
                att=torch.stack(out['attweights']).detach(), grads=grads)


def on(t, dtype=np.float64):
    return t.detach().cpu().numpy().astype(dtype)


class Arbiter(object):
    """fp64 CPU evaluation of the loop, computed on the first miss only."""

    def __init__(self, dec, batch):
        self.dec, self.batch, self.ref = dec, batch, None

    def get(self):
        if self.ref is None:
            dec64 = make_like(self.dec).double()
            enc, lens, texts, tl = self.batch
            self.ref = run(dec64, enc.double().cpu(), lens, texts, tl, native=False)
        return self.ref


def make_like(dec):
    import copy
    return copy.deepcopy(dec).cpu()


def close_abs(name, got, want, atol, arb, pick):
    err = np.abs(on(got) - on(want)).max() if got.numel() else 0.0
    if err <= atol:
        return
    ref = on(pick(arb.get()))
    e_native = np.abs(on(got) - ref).max()
    e_loop = np.abs(on(want) - ref).max()
    assert e_native <= max(atol, 2 * e_loop), (name, err, e_native, e_loop)


def close_norm(name, got, want, rtol, arb, pick, floor=1e-6):
    g, w = on(got), on(want)
    scale = max(np.linalg.norm(w), floor / rtol)
    err = np.linalg.norm(g - w)
    if err <= rtol * scale:
        return
    ref = on(pick(arb.get()))
    e_native, e_loop = np.linalg.norm(g - ref), np.linalg.norm(w - ref)
    assert e_native <= max(rtol * scale, 2 * e_loop), (name, err / scale, e_native, e_loop)


def compare(dec, batch, rtol_grad=1e-4):
    enc, lens, texts, tl = batch
    dec = dec.to(DEV)
    args = (enc.to(DEV), lens, texts, tl)
    got = run(dec, *args, native=True)
    want = run(dec, *args, native=False)
    arb = Arbiter(dec, batch)
    assert got['out']['loss'].grad_fn is not None
    np.testing.assert_allclose(float(got['loss']), float(want['loss']), rtol=1e-5)
    close_abs('logits', got['logits'], want['logits'], 1e-5, arb, lambda r: r['logits'])
    close_abs('alignments', got['att'], want['att'], 1e-5, arb, lambda r: r['att'])
    assert set(got['grads']) == set(want['grads'])
    for name in want['grads']:
        close_norm(name, got['grads'][name], want['grads'][name], rtol_grad, arb,
                   lambda r, n=name: r['grads'][n])
    return got


def recipe_batch(T=334, B=20):
    lens = [T - 8 * b for b in range(B)]
    text_lens = [100 - 5 * b for b in range(B)]
    text_lens[-1] = 0                                  # EOS only
    return make_batch(T, lens, text_lens)


@pytest.mark.gpu
def test_scan_matches_loop_at_recipe_dims():
    dec = make_decoder()
    assert dec.to(DEV)._native_train_ok(torch.zeros(334, 1, E, device=DEV))
    compare(dec, recipe_batch())


@pytest.mark.gpu
def test_scan_matches_loop_in_train_mode_without_dropout():
    dec = make_decoder(seed=5).train()
    compare(dec, recipe_batch(T=150, B=6))


def autograd_nodes(t):
    seen, stack, names = set(), [t.grad_fn], []
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        names.append(type(n).__name__)
        stack.extend(f for f, _ in n.next_functions)
    return names


@pytest.mark.gpu
def test_native_path_runs_as_one_node():
    dec = make_decoder().to(DEV)
    counts = {}
    for native in (True, False):
        os.environ[SWITCH] = '1' if native else '0'
        try:
            for top in (10, 100):                      # L = 11 and L = 101
                enc, lens, texts, tl = make_batch(120, [120, 100, 90], [top, top // 2, 3])
                loss = dec(enc.to(DEV).requires_grad_(), lens, texts, tl)['loss']
                names = autograd_nodes(loss)
                counts[native, top] = len(names)
                if native:
                    assert '_AttentionScanBackward' in names
                else:
                    assert '_AttentionScanBackward' not in names
        finally:
            os.environ.pop(SWITCH, None)
    assert counts[True, 10] == counts[True, 100]
    assert counts[False, 100] > counts[False, 10]       # the loop grows with L


EDGE = {
    'B1': dict(A=64, T=50, lens=[50], tl=[7]),
    'short_len1_text0': dict(A=64, T=20, lens=[20, 13, 1], tl=[0, 4, 9]),
    'A8': dict(A=8, T=90, lens=[90, 61, 33, 5], tl=[12, 40, 0, 3]),
    'A256': dict(A=256, T=120, lens=[120, 77, 40], tl=[30, 9, 17]),
    'no_learnable_init': dict(A=64, T=77, lens=[77, 70, 31, 12], tl=[20, 5, 11, 0],
                              learnable=False),
    'T2000': dict(A=64, T=2000, lens=[2000, 1500], tl=[30, 12]),
    'T4096_limit': dict(A=64, T=4096, lens=[4096], tl=[6]),
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(EDGE))
def test_scan_edge_cases(case):
    c = EDGE[case]
    dec = make_decoder(A=c['A'], learnable=c.get('learnable', True), seed=7)
    batch = make_batch(c['T'], c['lens'], c['tl'], seed=11)
    assert dec.to(DEV)._native_train_ok(batch[0].to(DEV))
    compare(dec, batch)


@pytest.mark.gpu
def test_scan_beyond_the_limit_takes_the_loop():
    dec = make_decoder().to(DEV)
    assert not dec._native_train_ok(torch.zeros(4097, 1, E, device=DEV))


@pytest.mark.gpu
def test_scan_is_bitwise_reproducible():
    dec = make_decoder().to(DEV)
    enc, lens, texts, tl = recipe_batch()
    a = run(dec, enc.to(DEV), lens, texts, tl, native=True)
    b = run(dec, enc.to(DEV), lens, texts, tl, native=True)
    assert torch.equal(a['loss'], b['loss'])
    assert torch.equal(a['att'], b['att'])
    for name in a['grads']:
        assert torch.equal(a['grads'][name], b['grads'][name]), name


@pytest.mark.gpu
def test_stage2_speech_model_trains_through_the_scan():
    """A whole stage-2 SpeechModel (DeepSpeech2 encoder + AttentionDecoderTCN, tcn.yaml
    model section, dropout 0) at a small batch: the first step's loss and gradients match the
    loop's, and three Adam steps lower the loss."""
    import bench
    from att_speech.models import SpeechModel
    B, T = 4, 240
    feats, lens, texts, llens = bench.synthetic_batch(B, T, 0, 1)
    texts, llens = texts[:, :40].contiguous(), torch.clamp(llens - 60, min=0)
    for b in range(B):
        texts[b, int(llens[b]):] = 0
    enc_cfg, _ = bench.model_config(1, None)
    dec_cfg = dict(class_name='att_speech.modules.tcn.AttentionDecoderTCN', att_hidden_size=64,
                   attention_temperature=1.25, beam_size=1, branching_threshold=0.0,
                   dilation_sizes=[1, 2], dropout_p=0.0, kernel_size=3,
                   length_normalization=0.6, tcn_hidden_size=384, tcn_layers_per_block=2)
    sample = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(),
              'spkids': None}
    torch.manual_seed(0)
    model = SpeechModel(enc_cfg, dec_cfg, sample, S, [str(i) for i in range(S)]).to(DEV)
    with torch.no_grad():
        model.decoder.attn.hidden_to_score.weight.normal_(0.0, 0.5)
    f = feats.to(DEV)
    d_encoded = []

    def keep_grad(module, inputs, output):
        output[0].register_hook(lambda g: d_encoded.append(g.detach().clone()))
    model.encoder.register_forward_hook(keep_grad)

    def step(native):
        os.environ[SWITCH] = '1' if native else '0'
        try:
            model.zero_grad(set_to_none=True)
            loss = model(f, lens, None, texts, llens)['loss']
            loss.backward()
        finally:
            os.environ.pop(SWITCH, None)
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
                 if p.grad is not None}
        grads['d_encoded'] = d_encoded.pop()
        return float(loss), grads

    loss_loop, g_loop = step(False)
    loss_nat, g_nat = step(True)
    np.testing.assert_allclose(loss_nat, loss_loop, rtol=1e-5)
    assert set(g_nat) == set(g_loop)
    for name in g_loop:
        # the encoder's own backward is bf16 (convolutions, LSTM recurrence): the ~1e-6
        # difference in d encoded moves its parameter gradients by whole bf16 roundings
        rtol = 1e-2 if name.startswith('encoder.') else 1e-4
        w, g = on(g_loop[name]), on(g_nat[name])
        scale = max(np.linalg.norm(w), 1e-6 / rtol)
        assert np.linalg.norm(g - w) <= rtol * scale, (name, np.linalg.norm(g - w) / scale)
    opt = torch.optim.Adam(model.parameters(), lr=4e-4)
    losses = []
    os.environ[SWITCH] = '1'
    try:
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            loss = model(f, lens, None, texts, llens)['loss']
            loss.backward()
            opt.step()
            losses.append(float(loss))
    finally:
        os.environ.pop(SWITCH, None)
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0], losses
