"""The recipes' weight-noise and KillOnNan hooks on the device: the counter-based noise kernel
(csrc/noise.hip: asr_gaussian_noise_f32) against the numpy Philox4x32-10 + Box-Muller statement
of att_speech.noise, its apply / remove round trip, the weight-noise hook on small GPU
SpeechModels (mono-char LutLinear, bi-char CDE), FusedClipAdam with a device-mode KillOnNan
against the host hooks + torch.optim.Adam, and two ranks over gloo that noise and skip together."""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SENTINEL = 7.25


def _segments(ce):
    """(offset in the buffer, global index, count): starts not multiples of 4, counts 1, 3, chunk+1;
    the last piece is 16-byte aligned for its groups of four"""
    return [(1, 5, 1), (10, 7, 3), (101, 1002, ce + 1), (ce + 1203, (1 << 33) + 3, 257),
            (ce + 1601, 40, 4096), (2 * ce + 5702, 0, 9), (4 * ce, 8, 2001)]


def _views(buf, segs):
    return [buf[o:o + c] for o, _, c in segs], [i for _, i, _ in segs]


def test_kernel_draw_matches_the_checker():
    from att_speech import _native, noise
    dev = torch.device('cuda:0')
    ce = _native.lib().asr_noise_chunk_elems()
    segs = _segments(ce)
    n = max(o + c for o, _, c in segs) + 17
    seed, it = 0x1234567890ABCDEF, 20001
    buf = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    views, starts = _views(buf, segs)
    noise.write_normal(views, starts, seed, 0, it)
    got = buf.cpu().numpy()
    inside = np.zeros(n, bool)
    for o, i0, c in segs:
        inside[o:o + c] = True
        want = noise.normal_f64(np.arange(i0, i0 + c, dtype=np.uint64), seed, 0, it)
        assert np.abs(got[o:o + c] - want).max() <= 1e-5, (o, i0, c)
    assert np.all(got[~inside] == SENTINEL)
    # same key: the same bits; another iteration, tag or seed: other numbers
    again = torch.full_like(buf, SENTINEL)
    noise.write_normal(_views(again, segs)[0], starts, seed, 0, it)
    assert torch.equal(again, buf)
    for s2, t2, it2 in ((seed, 0, it + 1), (seed, 1, it), (seed + 1, 0, it), (seed ^ (1 << 40), 0, it)):
        other = torch.full_like(buf, SENTINEL)
        noise.write_normal(_views(other, segs)[0], starts, s2, t2, it2)
        diff = (other != buf)[torch.from_numpy(inside).to(dev)]
        assert float(diff.float().mean()) > 0.99


def test_kernel_moments():
    from att_speech import noise
    dev = torch.device('cuda:0')
    n = 1 << 24
    z = torch.empty(n, dtype=torch.float32, device=dev)
    noise.write_normal([z], [0], 987654321, 0, 3)
    z = z.double()
    mean, var = float(z.mean()), float(z.var())
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1) <= 5 * np.sqrt(2.0 / n)
    p = 0.0026997960632601866            # P(|z| > 3)
    tail = float((z.abs() > 3).double().mean())
    assert abs(tail - p) <= 5 * np.sqrt(p * (1 - p) / n)


def test_apply_and_remove_round_trip():
    from att_speech import _native, noise
    dev = torch.device('cuda:0')
    ce = _native.lib().asr_noise_chunk_elems()
    segs = _segments(ce)
    n = max(o + c for o, _, c in segs) + 17
    seed, it = 42, 7
    sigmas = [0.15, 0.3, 1e-3, 2.5, 0.15, 0.07, 0.5]
    g = torch.Generator().manual_seed(0)
    w0 = torch.randn(n, generator=g).to(dev)
    inside = torch.zeros(n, dtype=torch.bool, device=dev)
    for o, _, c in segs:
        inside[o:o + c] = True
    w0[~inside] = SENTINEL
    # the kernel's own z
    z = torch.zeros(n, dtype=torch.float32, device=dev)
    noise.write_normal(_views(z, segs)[0], [i for _, i, _ in segs], seed, 0, it)
    r = torch.zeros_like(z)
    for (o, _, c), s in zip(segs, sigmas):
        r[o:o + c] = z[o:o + c] * torch.tensor(s, dtype=torch.float32, device=dev)
    w = w0.clone()
    tab = noise.SegmentTable()
    views, starts = _views(w, segs)
    table, nsegs = tab.get(views, starts, sigmas)
    noise.launch(table, nsegs, seed, 0, it, sign=1)
    plus = w0 + r
    assert torch.equal(w, plus)
    noise.launch(table, nsegs, seed, 0, it, sign=-1)
    assert torch.equal(w, plus + (-r))
    assert torch.equal(w[~inside], w0[~inside])


# ------------------------------------------------------------------------------------------
# the hook on small GPU SpeechModels
# ------------------------------------------------------------------------------------------
def _speech_model(order, workload):
    import bench
    from att_speech.models import SpeechModel
    dev = torch.device('cuda:0')
    feats, lens, texts, llens = bench.synthetic_batch(4, 700, 0, order)
    enc_cfg, dec_cfg = bench.model_config(order, workload)
    torch.manual_seed(7)
    sb = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(), 'spkids': None}
    model = SpeechModel(enc_cfg, dec_cfg, sb, 49 ** order, [str(i) for i in range(49)]).to(dev)
    return model, (feats.to(dev), lens, None, texts, llens)


@pytest.mark.parametrize('workload', ['ctc', 'ctcg_bi_cde'])
def test_weight_noise_hook_on_speech_model(workload):
    from att_speech import noise
    from att_speech.modules.hooks import LinearIncreaseWeightNoise
    order = 1 if workload == 'ctc' else 2
    model, args = _speech_model(order, None if workload == 'ctc' else workload)
    supporting = [] if workload == 'ctc' else ['decoder.fc.0.module.0']
    twin = copy.deepcopy(model)
    w0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    it, seed = 12000, 77
    hook = LinearIncreaseWeightNoise({'decoder': 0.15, 'encoder': 0.1}, 20000,
                                     modules_supporting_noise=supporting, seed=seed)
    noised = [(n, p) for n, p in model.named_parameters() if hook._requires_noise(n)]
    assert any('rnn' in n for n, _ in noised) and any('conv' in n for n, _ in noised)
    assert ('decoder.fc.0.module.0.weight' in dict(noised)) == (workload == 'ctc')
    # what the weights must be inside forward: w + sigma_it * z, z from the kernel itself
    want, start = {}, 0
    for n, p in noised:
        z = torch.empty_like(p)
        noise.write_normal([z], [start], seed, noise.TAG_WEIGHT, it)
        s = torch.tensor(hook.get_rand_val(n, it), dtype=torch.float32, device=p.device)
        want[n] = (w0[n] + z * s, z * s)
        start += p.numel()
    seen = {}

    def fwd(*a):
        seen.update({n: p.detach().clone() for n, p in model.named_parameters()})
        return model(*a)
    hook.pre_train_forward(model, None, it)
    if supporting:
        assert model.get_submodule(supporting[0]).weight_noise == pytest.approx(0.15 * 12000 / 20000)
    torch.manual_seed(5)
    loss = fwd(*args)['loss']
    loss.backward()
    hook.post_backward(model, None, it, loss)
    if supporting:
        assert model.get_submodule(supporting[0]).weight_noise == 0.0
    for n, p in model.named_parameters():
        if n in want:
            assert torch.equal(seen[n], want[n][0]), n
            assert torch.equal(p.detach(), want[n][0] + (-want[n][1])), n
        else:
            assert torch.equal(seen[n], w0[n]) and torch.equal(p.detach(), w0[n]), n
    # the gradients are those of a copy whose weights were set to the noised values by hand
    with torch.no_grad():
        for n, p in twin.named_parameters():
            if n in want:
                p.copy_(want[n][0])
    if supporting:
        twin.get_submodule(supporting[0]).weight_noise = hook.get_rand_val(supporting[0], it)
    torch.manual_seed(5)
    twin(*args)['loss'].backward()
    ga = torch.cat([p.grad.flatten() for p in model.parameters()])
    gb = torch.cat([p.grad.flatten() for p in twin.parameters()])
    assert torch.isfinite(ga).all()
    assert float((ga - gb).norm()) <= 1e-3 * float(gb.norm())


# ------------------------------------------------------------------------------------------
# FusedClipAdam with a device-mode KillOnNan
# ------------------------------------------------------------------------------------------
SHAPES = [(7,), (33, 65), (1024,), (1025,), (3, 700), (5000,), (2, 3, 4, 5)]


def test_fused_step_with_device_kill_on_nan_matches_host_hooks():
    from att_speech.dp import FlatGradBucket
    from att_speech.fused_step import FusedClipAdam
    from att_speech.modules.hooks import GradientClipping, KillOnNan
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(5)
    cpu = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    gpu = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in cpu]
    opt = torch.optim.Adam(cpu, lr=3e-3, betas=(0.9, 0.98), eps=1e-7)
    host_clip, host_kill = GradientClipping(50.0, 500.0), KillOnNan(priority=5)
    bucket = FlatGradBucket(gpu)
    kill = KillOnNan(priority=5)
    gopt = torch.optim.Adam(gpu, lr=3e-3, betas=(0.9, 0.98), eps=1e-7)
    fused = FusedClipAdam.from_optimizer(gopt, bucket, GradientClipping(50.0, 500.0), kill_on_nan=kill)
    assert kill.device_mode
    # (gradient scale, loss): finite, NaN, +inf, clipped, -inf, too large, finite
    nan, inf = float('nan'), float('inf')
    plan = [(0.1, 1.0), (0.1, nan), (0.2, inf), (3.0, 2.0), (0.1, -inf), (100.0, 1.0), (0.05, 3.0)]
    want = []
    for scale, lval in plan:
        grads = [torch.randn(*s, generator=g) * scale for s in SHAPES]
        for p, q, gr in zip(cpu, gpu, grads):
            p.grad = gr.clone()
            q.grad.copy_(gr)
        # host: trainer.py order, pre_backward hooks first; a skip stops the post_backward chain
        skip = host_kill.pre_backward(None, opt, 0, torch.tensor(lval))
        if skip:
            want.append(True)
        else:
            want.append(bool(host_clip.post_backward(_Params(cpu), opt, 0, None)))
            if not want[-1]:
                opt.step()
        # device
        assert kill.pre_backward(None, gopt, 0, torch.tensor(lval, device=dev)) is False
        assert kill.post_backward(None, gopt, 0, None) is False
        fused.step(None)
    got = fused.drain()
    assert [r[2] for r in got] == want == [False, True, True, False, True, True, False]
    assert all(len(r) == 4 for r in got)
    assert kill.grace_counter == host_kill.grace_counter == 7
    assert fused.steps_taken == 3
    for p, q in zip(cpu, gpu):
        np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().numpy(), rtol=2e-6, atol=2e-7)
    opt2 = torch.optim.Adam(gpu, lr=3e-3)
    fused.export_state(opt2)
    for p, q in zip(cpu, gpu):
        np.testing.assert_allclose(opt2.state[q]['exp_avg'].cpu().numpy(), opt.state[p]['exp_avg'].numpy(),
                                   rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(opt2.state[q]['exp_avg_sq'].cpu().numpy(), opt.state[p]['exp_avg_sq'].numpy(),
                                   rtol=2e-6, atol=1e-8)


class _Params(object):
    def __init__(self, params):
        self.params = params

    def get_parameters_for_optimizer(self):
        return self.params


def test_device_kill_on_nan_exits_after_the_tenth():
    from att_speech.dp import FlatGradBucket
    from att_speech.fused_step import FusedClipAdam
    from att_speech.modules.hooks import KillOnNan
    dev = torch.device('cuda:0')
    p = torch.nn.Parameter(torch.randn(100, device=dev))
    bucket = FlatGradBucket([p])
    kill = KillOnNan(priority=5)
    fused = FusedClipAdam(bucket, lr=1e-3, kill_on_nan=kill)
    bad = torch.tensor(float('nan'), device=dev)
    for _ in range(9):
        kill.pre_backward(None, None, 0, bad)
        fused.step(None)
    fused.drain()
    assert kill.grace_counter == 1
    kill.pre_backward(None, None, 0, bad)
    fused.step(None)
    with pytest.raises(SystemExit) as e:
        fused.drain()
    assert e.value.code == 1 and kill.grace_counter == 0


class _NoReadBack(object):
    """Tensor.item / __bool__ / __float__ / tolist raise for CUDA tensors while active."""
    NAMES = ('item', '__bool__', '__float__', 'tolist')

    def __enter__(self):
        self.saved = {n: getattr(torch.Tensor, n) for n in self.NAMES}
        for n, f in self.saved.items():
            def guard(t, *a, _f=f, _n=n, **k):
                if t.is_cuda:
                    raise AssertionError('read-back of a CUDA tensor (%s) inside a hook' % _n)
                return _f(t, *a, **k)
            setattr(torch.Tensor, n, guard)
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(torch.Tensor, n, f)


def _guarded(fn):
    def call(*a, **k):
        with _NoReadBack():
            return fn(*a, **k)
    return call


def _toy(dev):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4)).to(dev)


def test_recipe_hooks_in_train_step_read_nothing_back():
    from att_speech.dp import FlatGradBucket, train_step
    from att_speech.fused_step import FusedClipAdam
    from att_speech.modules.hooks import (GradientClipping, KillOnNan, LinearIncreaseWeightNoise,
                                          PolyakDecay)
    dev = torch.device('cuda:0')
    model = _toy(dev)
    bucket = FlatGradBucket(model.parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    hooks = sorted([GradientClipping(clip_norm=10000.0, skip_step_norm=100000.0), KillOnNan(priority=5),
                    LinearIncreaseWeightNoise(start_iteration=20, weight_noise=0.15), PolyakDecay([0.9998])],
                   key=lambda h: h.priority)
    for h in hooks:
        h.pre_run(model, opt)
    fused = FusedClipAdam.from_optimizer(opt, bucket, hooks[0], kill_on_nan=hooks[-1])
    for h in hooks:
        for name in ('pre_train_forward', 'pre_backward', 'post_backward', 'post_optimizer_step'):
            setattr(h, name, _guarded(getattr(h, name)))
    x = torch.randn(32, 8, device=dev)

    def fwd(x):
        return {'loss': (model(x) ** 2).sum()}
    for it in range(25, 29):
        train_step(model, opt, ((x,), {}), hooks=hooks, bucket=bucket, current_iteration=it, forward=fwd,
                   fused=fused)
    recs = fused.drain()
    assert len(recs) == 4 and not any(r[2] for r in recs)
    with _NoReadBack():
        with pytest.raises(AssertionError):
            x.sum().item()


# ------------------------------------------------------------------------------------------
# two ranks on one GPU over gloo
# ------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, 'pytorch-asr_amd')]
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from att_speech.dp import FlatGradBucket, train_step
    from att_speech.fused_step import FusedClipAdam
    from att_speech.modules.hooks import GradientClipping, KillOnNan, LinearIncreaseWeightNoise
    dev = torch.device('cuda:0')
    model = _toy(dev)                                       # the same initial replica...
    torch.manual_seed(100 + rank)                           # ...different torch generators
    torch.cuda.manual_seed(100 + rank)
    bucket = FlatGradBucket(model.parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    hooks = [GradientClipping(clip_norm=10000.0, skip_step_norm=100000.0),
             LinearIncreaseWeightNoise(start_iteration=2, weight_noise=0.1), KillOnNan(priority=5)]
    for h in hooks:
        h.pre_run(model, opt)
    fused = FusedClipAdam.from_optimizer(opt, bucket, hooks[0], kill_on_nan=hooks[2])
    g = torch.Generator().manual_seed(3 + rank)
    x = torch.randn(16, 8, generator=g).to(dev)
    seen = []

    def fwd(x, it):
        seen.append([p.detach().cpu().numpy().copy() for p in model.parameters()])
        loss = (model(x) ** 2).sum()
        if it == 2 and rank == 1:           # a NaN loss on rank 1 only, with finite gradients
            loss = loss + torch.tensor(float('nan'), device=dev)
        return {'loss': loss}
    for it in range(1, 5):
        train_step(model, opt, ((x, it), {}), hooks=hooks, bucket=bucket, current_iteration=it,
                   forward=fwd, fused=fused)
    recs = fused.drain()
    q.put((rank, seen, [r[2] for r in recs], hooks[2].grace_counter,
           [p.detach().cpu().numpy() for p in model.parameters()]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_noise_and_skip_together():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in procs:
        r = q.get(timeout=600)
        got[r[0]] = r[1:]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (seen0, skip0, cnt0, p0), (seen1, skip1, cnt1, p1) = got[0], got[1]
    for a, b in zip(seen0, seen1):                  # the weights inside every forward
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert skip0 == skip1 == [False, True, False, False]
    assert cnt0 == cnt1 == 9
    assert all(np.array_equal(x, y) for x, y in zip(p0, p1))
    assert not np.array_equal(seen0[1][0], seen0[2][0])     # noise at iteration 2 differs from 1
