"""AttentionDecoderRNN on the MI355X: the native label scan (asr_att_gru_scan_fwd_f32 / _bwd_f32
behind attention_decoder._AttentionGruScan) and the native decode loop.

Referee: this class evaluated in fp64 on the CPU.  Rule: the native result may
be at most twice as far from the fp64 values as the fp32 CPU evaluation of the same class is,
in the maximum and in the mean, with the project's floors — loss 1e-4 relative; alignments
(rows that sum to 1) 2e-5 max / 2e-6 mean; states and every gradient 1e-4 of the tensor's
largest magnitude."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import golden

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu

S, E = 49, 320
SWITCH = 'ASR_ATT_RNN_NATIVE'


def dev():
    return torch.device('cuda:0')


def decoder_class():
    from att_speech.modules.decoders.attention_decoder import AttentionDecoderRNN
    return AttentionDecoderRNN


def make_decoder(H=256, seed=0, E_=E, **kw):
    torch.manual_seed(seed)
    args = dict(n_layers=1, hidden_size=H, dropout_p=0.0)
    args.update(kw)
    dec = decoder_class()({'features': torch.zeros(4, 2, E_)}, S, **args)
    with torch.no_grad():
        dec.attn.hidden_to_score.weight.normal_(0.0, 0.5)      # peaky, moving alignments
        dec.rnn_zero_state.normal_(0.0, 0.3)
        dec.output_to_logits.bias.normal_(0.0, 0.3)
    return dec


def make_batch(T, lens, text_lens, seed=1, E_=E):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    enc = torch.randn(T, B, E_, generator=g)
    texts = torch.randint(2, S, (B, max(max(text_lens), 1)), generator=g, dtype=torch.int32)
    for b, n in enumerate(text_lens):
        texts[b, n:] = 0
    return enc, torch.tensor(lens, dtype=torch.int32), texts, torch.tensor(text_lens)


def run(dec, enc, lens, texts, text_lens, native=True):
    os.environ[SWITCH] = '1' if native else '0'
    try:
        dec.zero_grad(set_to_none=True)
        x = enc.clone().requires_grad_()
        out = dec(x, lens, texts, text_lens, return_att_weights=True, return_rnn_states=True)
        out['loss'].backward()
    finally:
        os.environ.pop(SWITCH, None)
    grads = {n: p.grad.detach().clone() for n, p in dec.named_parameters() if p.grad is not None}
    grads['d_encoded'] = x.grad.detach().clone()
    return dict(out=out, loss=out['loss'].detach(), att=torch.stack(out['attweights']).detach(),
                states=torch.stack(out['rnnstates']).detach(), grads=grads)


def on(t):
    return t.detach().cpu().numpy().astype(np.float64)


def cpu_runs(dec, batch):
    """-> (fp64 referee, fp32 CPU evaluation) of the same module and inputs"""
    enc, lens, texts, tl = batch
    ref = run(copy.deepcopy(dec).cpu().double(), enc.double(), lens, texts, tl)
    f32 = run(copy.deepcopy(dec).cpu(), enc, lens, texts, tl)
    return ref, f32


def judge(name, got, f32, ref, floor_max, floor_mean, report):
    g, c, r = on(got), on(f32), on(ref)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    e_nat, e_cpu = np.abs(g - r), np.abs(c - r)
    report.append('%-40s native max %.3e mean %.3e | cpu32 max %.3e mean %.3e | floors %.1e %.1e' % (
        name, e_nat.max(), e_nat.mean(), e_cpu.max(), e_cpu.mean(), floor_max, floor_mean))
    return (e_nat.max() <= max(floor_max, 2 * e_cpu.max())
            and e_nat.mean() <= max(floor_mean, 2 * e_cpu.mean()))


def arbitrate(got, f32, ref):
    """the rule of the module docstring over loss, alignments, states and every gradient"""
    report, bad = [], []

    def check(name, a, b, c, fmax, fmean):
        if not judge(name, a, b, c, fmax, fmean, report):
            bad.append(name)
    check('loss', got['loss'], f32['loss'], ref['loss'], 1e-4 * abs(float(ref['loss'])),
          1e-4 * abs(float(ref['loss'])))
    check('alignments', got['att'], f32['att'], ref['att'], 2e-5, 2e-6)
    scale = float(ref['states'].abs().max())
    check('states', got['states'], f32['states'], ref['states'], 1e-4 * scale, 1e-4 * scale)
    assert set(got['grads']) == set(ref['grads'])
    for name in sorted(ref['grads']):
        scale = float(ref['grads'][name].abs().max())
        check('grad ' + name, got['grads'][name], f32['grads'][name], ref['grads'][name],
              1e-4 * scale, 1e-4 * scale)
    print('\n'.join(report))
    assert not bad, (bad, report)


def to_dev(batch):
    return (batch[0].to(dev()),) + tuple(batch[1:])


# ------------------------------------------------------------------------------- fixture
def fixture_decoder(g, **kw):
    T, B, E_ = g['enc'].shape
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd_')}
    args = dict(n_layers=1, hidden_size=sd['rnn_zero_state'].shape[2], dropout_p=0.0,
                beam_size=3, length_normalization=float(g['length_normalization']))
    args.update(kw)
    dec = decoder_class()({'features': torch.zeros(T, B, E_)}, int(g['S']), **args)
    dec.load_state_dict(sd)
    return dec


def test_fixture_parity_on_the_device():
    """native forward + backward against the numbers the reference's own class recorded"""
    g = golden('attention_rnn.npz')
    dec = fixture_decoder(g).to(dev())
    enc = torch.from_numpy(g['enc']).to(dev())
    assert dec._native_train_ok(enc)
    got = run(dec, enc, torch.from_numpy(g['lens']), torch.from_numpy(g['texts']),
              torch.from_numpy(g['text_lens']))
    assert '_AttentionGruScanBackward' in autograd_nodes(got['out']['loss'])

    def close(name, a, want, rtol):
        a, want = on(a), np.asarray(want, np.float64)
        assert a.shape == want.shape, name
        err = np.abs(a - want).max() / max(np.abs(want).max(), 1e-30)
        print('%-40s %.3e' % (name, err))
        assert err <= rtol, (name, err)
    close('loss', got['loss'], g['loss'], 1e-4)
    assert np.abs(on(got['att']) - g['att']).max() <= 2e-5
    close('states', got['states'], g['states'], 1e-4)
    for name in got['grads']:
        key = 'grad_encoded' if name == 'd_encoded' else 'grad_' + name
        if name == 'attn.hidden_to_score.bias':
            # exactly zero by shift invariance; the reference's is its own rounding noise
            assert float(got['grads'][name].abs().max()) <= 1e-6
            continue
        close(key, got['grads'][name], g[key], 1e-4)


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


# ------------------------------------------------------------------------------- real sizes
def uneven(top, B, low=1):
    return [max(low, top - (top * b) // max(B, 1)) for b in range(B)]


CASES = {
    # B = 20 at the stage-2 shapes; one utterance of ONE frame, one EOS-only label sequence
    'H256_B20_T334_L101': dict(H=256, T=334, lens=uneven(334, 19) + [1],
                               tl=[100] + uneven(90, 18) + [0]),
    'H128_B5_T334_L41': dict(H=128, T=334, lens=[334, 300, 211, 64, 1], tl=[40, 0, 17, 33, 5]),
    'H320_B1_T334_L31': dict(H=320, T=334, lens=[334], tl=[30]),
    'H320_B5_T150_L26': dict(H=320, T=150, lens=[150, 149, 65, 64, 63], tl=[25, 3, 0, 12, 25]),
    'H256_B1_T77_L1': dict(H=256, T=77, lens=[50], tl=[0]),
    'H128_B20_T150_L13': dict(H=128, T=150, lens=uneven(150, 20), tl=uneven(12, 20, low=0)),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_scan_against_the_fp64_referee(case):
    c = CASES[case]
    dec = make_decoder(H=c['H'], seed=3)
    batch = make_batch(c['T'], c['lens'], c['tl'], seed=11)
    ref, f32 = cpu_runs(dec, batch)
    dec = dec.to(dev())
    assert dec._native_train_ok(batch[0].to(dev()))
    got = run(dec, *to_dev(batch))
    assert '_AttentionGruScanBackward' in autograd_nodes(got['out']['loss'])
    arbitrate(got, f32, ref)
    # rows sum to 1; exactly zero beyond each utterance's length
    att = got['att']                                                       # [L, T, B]
    assert float((att.sum(1) - 1).abs().max()) <= 3e-6
    for b, n in enumerate(c['lens']):
        assert not bool((att[:, n:, b] != 0).any())
    # native == loop on the device, by the same rule (the loop in the fp32 CPU's place)
    loop = run(dec, *to_dev(batch), native=False)
    assert '_AttentionGruScanBackward' not in autograd_nodes(loop['out']['loss'])
    arbitrate(got, loop, ref)


def test_scan_is_bitwise_reproducible():
    c = CASES['H256_B20_T334_L101']
    dec = make_decoder(H=c['H'], seed=3).to(dev())
    batch = to_dev(make_batch(c['T'], c['lens'], c['tl'], seed=11))
    a, b = run(dec, *batch), run(dec, *batch)
    assert torch.equal(a['loss'], b['loss'])
    assert torch.equal(a['att'], b['att']) and torch.equal(a['states'], b['states'])
    for name in a['grads']:
        assert torch.equal(a['grads'][name], b['grads'][name]), name


@pytest.mark.parametrize('kw', [dict(n_layers=2), dict(att_force_forward=(-2, 12))])
def test_outside_the_gate_the_switch_changes_no_bit(kw):
    dec = make_decoder(H=128, seed=5, **kw).to(dev())
    batch = to_dev(make_batch(90, [90, 61, 33], [12, 0, 7], seed=2))
    assert not dec._native_train_ok(batch[0])
    a, b = run(dec, *batch, native=True), run(dec, *batch, native=False)
    assert '_AttentionGruScanBackward' not in autograd_nodes(a['out']['loss'])
    assert torch.equal(a['loss'], b['loss']) and torch.equal(a['att'], b['att'])


def test_beyond_the_limits_takes_the_loop():
    dec = make_decoder().to(dev())
    assert not dec._native_train_ok(torch.zeros(4097, 1, E, device=dev()))
    assert not make_decoder(H=324).to(dev())._native_train_ok(torch.zeros(8, 1, E, device=dev()))


# ------------------------------------------------------------------------------- decoding
def labels_of(res):
    return [[int(c) for c in (d.tolist() if hasattr(d, 'tolist') else d)] for d in res['decoded']]


@pytest.mark.parametrize('beam', [1, 3])
def test_native_decode_returns_the_fixture(beam):
    g = golden('attention_rnn.npz')
    dec = fixture_decoder(g, beam_size=beam).to(dev()).eval()
    dec.TRANSCRIPTION_LEN_GUARD = int(g['guard'])
    enc = torch.from_numpy(g['enc']).to(dev())
    assert dec._native_decode_ok(enc)
    with torch.no_grad():
        res = dec.decode(enc, torch.from_numpy(g['lens']))
    key = 'dec%d_' % beam
    got = labels_of(res)
    assert [len(d) for d in got] == g[key + 'lens'].tolist()
    assert [c for d in got for c in d] == g[key + 'flat'].tolist()
    np.testing.assert_allclose(res['decoded_scores']['acoustic'], g[key + 'scores'], rtol=1e-4)
    np.testing.assert_allclose(float(res['loss']), float(g[key + 'loss']), rtol=1e-4)


def watched_search(margins):
    """BeamSearch that records, per utterance, the smallest decision margin of the search:
    last kept against first dropped candidate, and EOS against the best other class of every
    live hypothesis."""
    from att_speech.modules.beam_search import BeamSearch

    class Watched(BeamSearch):
        def step(self, logits, *args, **kwargs):
            B, beam, C = self.batch_size, self.beam_size, self.num_classes
            gs = torch.log_softmax(logits.squeeze(0), 1) + self.scores[:, None]
            worst = torch.full((B,), float('inf'), device=gs.device)
            if self.estimations is not None:
                gap = (gs[:, -1] - gs[:, :-1].max(1)[0]).abs()
                gap = torch.where(torch.isfinite(self.scores), gap, torch.full_like(gap, float('inf')))
                worst = torch.minimum(worst, gap.view(B, beam).min(1)[0])
            cand = gs[:, :-1].contiguous().view(B, -1)
            if self.estimations is None:
                cand = cand[:, :C - 1]
            top = torch.sort(cand, 1, descending=True)[0]
            gap = top[:, beam - 1] - top[:, beam]
            worst = torch.minimum(worst, torch.where(torch.isfinite(gap), gap,
                                                     torch.full_like(gap, float('inf'))))
            margins.append(worst.cpu())
            return super(Watched, self).step(logits, *args, **kwargs)
    return Watched


DECODE_SEED = 8      # 16 of 16 utterances have clear margins on the host path (CPU check)


def decode_model():
    dec = make_decoder(H=256, seed=DECODE_SEED, beam_size=10, length_normalization=0.6)
    with torch.no_grad():
        dec.embedding.weight.mul_(2.0)
        dec.output_to_logits.weight.mul_(10.0)   # spread scores: few near-ties
        dec.output_to_logits.bias[S] += 2.0
    dec.TRANSCRIPTION_LEN_GUARD = 8           # 8 steps x beam 10: few enough decisions
    return dec.eval()


def test_native_decode_matches_the_host_search(monkeypatch):
    from att_speech.modules.decoders import attention_decoder
    B = 16
    dec = decode_model().to(dev())
    enc, lens, _, _ = make_batch(120, uneven(120, B, low=20), [1] * B, seed=DECODE_SEED)
    enc = enc.to(dev())
    margins = []
    monkeypatch.setattr(attention_decoder, 'BeamSearch', watched_search(margins))
    monkeypatch.setenv(SWITCH, '0')
    with torch.no_grad():
        host = dec.decode(enc, lens)
    monkeypatch.setenv(SWITCH, '1')
    assert dec._native_decode_ok(enc)
    with torch.no_grad():
        native = dec.decode(enc, lens)
    clear = torch.stack(margins).min(0)[0] > 1e-3
    print('utterances with clear margins: %d / %d' % (int(clear.sum()), B))
    assert int(clear.sum()) >= 0.9 * B
    want, got = labels_of(host), labels_of(native)
    assert any(len(d) > 1 for d in want)
    for b in range(B):
        if clear[b]:
            assert got[b] == want[b], (b, got[b], want[b])
            np.testing.assert_allclose(native['decoded_scores']['acoustic'][b],
                                       host['decoded_scores']['acoustic'][b], rtol=1e-4)


# ------------------------------------------------------------------------------- whole model
def test_speech_model_trains_through_the_scan():
    """DeepSpeech2 encoder + this decoder, dp.train_step with FusedClipAdam: the scan is in
    the graph and five steps on a fixed batch lower the loss."""
    import bench
    from att_speech.dp import FlatGradBucket, train_step
    from att_speech.fused_step import FusedClipAdam
    from att_speech.models import SpeechModel
    from att_speech.modules.hooks import GradientClipping
    B, T = 4, 240
    feats, lens, texts, llens = bench.synthetic_batch(B, T, 0, 1)
    texts, llens = texts[:, :30].contiguous(), torch.clamp(llens, max=30)
    for b in range(B):
        texts[b, int(llens[b]):] = 0
    enc_cfg, _ = bench.model_config(1, None)
    dec_cfg = dict(class_name='att_speech.modules.decoders.attention_decoder.AttentionDecoderRNN',
                   n_layers=1, hidden_size=256, dropout_p=0.2, beam_size=1)
    sample = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(), 'spkids': None}
    torch.manual_seed(0)
    model = SpeechModel(enc_cfg, dec_cfg, sample, S, [str(i) for i in range(S)]).to(dev())
    f = feats.to(dev())
    loss = model(f, lens, None, texts, llens)['loss']
    assert '_AttentionGruScanBackward' in autograd_nodes(loss)
    bucket = FlatGradBucket(model.parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    hook = GradientClipping(clip_norm=100.0, skip_step_norm=1e6)
    hook.pre_run(model, opt)
    fused = FusedClipAdam.from_optimizer(opt, bucket, hook)
    losses = []
    for _ in range(5):
        out, skip = train_step(model, opt, ((f, lens, None, texts, llens), {}), hooks=[hook],
                               bucket=bucket, fused=fused)
        assert not skip
        losses.append(float(out['loss'].detach()))
    fused.drain()
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0], losses
