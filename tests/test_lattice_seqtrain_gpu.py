"""asr_lattice_seqtrain_f64 (csrc/lattice_train.hip) through DeviceLatticeBatch.seq_objective,
att_speech.lattice_train.lattice_objective and the loss modules of att_speech.modules.sequence_losses, on the
GPU: the device against the numpy twin (which tests/test_lattice_seqtrain.py holds against brute-force
enumeration), the scatter bit for bit, repeatability, the refusals, the switch and the losses end to end.

Tolerance, device against twin: 1e-9 max(1, T_b) on the objective and on every arc_grad, both fp64 as the
launch returns them (T_b: the utterance's frames; a path's accuracy, and so the sMBR values, grow with it)."""
import numpy as np
import pytest
import torch

import nbest_cases
import seqtrain_cases as cases
from test_lattice_gpu import RTOL_LOSS, grad_atol

from att_speech import lattice_dp
from att_speech.lattice_dp import DeviceLatticeBatch
from att_speech.lattice_train import lattice_objective
from att_speech.modules.sequence_losses import LatticeMMILoss, LatticeSMBRLoss, ctc_loglik
from att_speech.wfst_lattice import LatticeBatch

pytestmark = pytest.mark.gpu

INF = float('inf')
LM = 1.25
_BATCH, _TWIN = {}, {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device('cuda:0')


def load(key):
    kind = key[0]
    if kind == 'toy':
        return cases.toy_case(*key[1:])
    if kind == 'unq':
        return cases.unquantised_case(key[1])
    return cases.fan_case() if kind == 'fan' else cases.mixed_case()


def device_case(key):
    """(DeviceLatticeBatch on the GPU, LatticeBatch, log_probs and ref as device tensors, lp, ref); the toys'
    scores are NaN beyond an utterance's frames, on the device too: they must never be read"""
    if key not in _BATCH:
        lats, lp, ref = load(key)
        d = dev()
        _BATCH[key] = (DeviceLatticeBatch.from_lattices(lats, d), LatticeBatch(lats),
                       torch.from_numpy(lp).to(d), torch.from_numpy(ref).to(d), lp, ref)
    return _BATCH[key]


def twin(key, criterion, boost, scale=None, use_ref=True):
    k = (key, criterion, boost, scale, use_ref)
    if k not in _TWIN:
        _, hb, _, _, lp, ref = device_case(key)
        _TWIN[k] = hb.seq_objective(lp, ref if use_ref else None, criterion, scale, LM, boost)
    return _TWIN[k]


def launch(key, criterion, boost, scale=None, use_ref=True, **kw):
    batch, _, lp_d, ref_d, _, _ = device_case(key)
    out = batch.seq_objective(lp_d, ref_d if use_ref else None, criterion, scale, LM, boost, **kw)
    assert out[0].dtype == torch.float64 and out[1].dtype == torch.float64 and out[2].dtype == torch.float32
    assert all(x.is_cuda for x in out) and out[2].shape == lp_d.shape
    return [x.cpu().numpy() for x in out]


def segment_sums(batch, arc_grad, shape):
    """float32 of arc_grad summed per (frame, class) in ascending arc order in fp64 on the host"""
    arrays = (batch.ilabel.cpu().numpy(), batch.time.cpu().numpy()[batch.dst_global.cpu().numpy()],
              batch.arc_utt.cpu().numpy())
    return cases.arc_sums(arrays, arc_grad, *shape).astype(np.float32)


def check_case(key, scale=None, use_ref=True):
    batch, hb, lp_d, _, _, _ = device_case(key)
    frames = np.maximum(1, batch.num_frames).astype(np.float64)
    for criterion in cases.CRITERIA:
        for boost in cases.BOOSTS:
            what = (key, criterion, boost)
            obj, arc_grad, occ = launch(key, criterion, boost, scale, use_ref)
            w_obj, w_grad, _ = twin(key, criterion, boost, scale, use_ref)
            fin = np.isfinite(w_obj)
            assert (np.isfinite(obj) == fin).all() and (obj[~fin] == w_obj[~fin]).all(), what
            assert (np.abs(obj[fin] - w_obj[fin]) <= 1e-9 * frames[fin]).all(), (what, obj, w_obj)
            tol = 1e-9 * frames[batch.arc_utt.cpu().numpy()] if len(arc_grad) else 0.0
            assert (np.abs(arc_grad - w_grad) <= tol).all(), (what, float(np.abs(arc_grad - w_grad).max()))
            # the scatter, bit for bit: the device's own arc_grad, summed on the host
            assert (occ == segment_sums(batch, arc_grad, tuple(lp_d.shape))).all(), what
            assert batch.launches == 1


@pytest.mark.parametrize('name', sorted(nbest_cases.TOYS))
def test_device_against_twin_on_the_toy_sweep(name):
    for scale in nbest_cases.SCALES:
        for lb in nbest_cases.LATTICE_BEAMS:
            check_case(('toy', name, scale, lb))
    # single-path lattices: the sMBR derivative is exactly zero on the device too
    key = ('toy', name, 1.0, 0.0)
    counts = [len(cases.complete_paths(l)[0]) for l in load(key)[0]]
    _, arc_grad, occ = launch(key, 'smbr', 0.5)
    utt = device_case(key)[0].arc_utt.cpu().numpy()
    assert (arc_grad[np.isin(utt, np.nonzero(np.array(counts) == 1)[0])] == 0).all()


@pytest.mark.parametrize('lb', nbest_cases.UNQUANTISED_BEAMS)
def test_device_against_twin_on_the_unquantised_bigram(lb):
    check_case(('unq', lb))
    check_case(('unq', lb), scale=0.7)


def test_device_against_twin_on_the_fan_lattice():
    check_case(('fan',))


def test_device_against_twin_on_the_mixed_batch():
    check_case(('mixed',))
    obj, arc_grad, occ = launch(('mixed',), 'mmi', 0.5)
    assert obj[1] == -INF and (occ[:, 1] == 0).all()
    assert launch(('mixed',), 'smbr', 0.5)[0][1] == 0.0


def test_device_without_a_reference():
    check_case(('toy', 'b', 1.0, 4.0), use_ref=False)
    obj, arc_grad, occ = launch(('toy', 'b', 1.0, 4.0), 'smbr', 0.5, use_ref=False)
    assert (obj == 0).all() and (arc_grad == 0).all() and (occ == 0).all()


def test_mmi_on_the_decode_scores_is_the_posterior_launch():
    """with the scores the lattice was decoded from, 'mmi' agrees with asr_lattice_posterior_f64"""
    lats = nbest_cases.unquantised_lattices(4.0)
    batch = DeviceLatticeBatch.from_lattices(lats, dev())
    lp = nbest_cases.unquantised_scores().to(dev())
    post = batch.posteriors(0.8, LM)
    obj, arc_grad, occ = batch.seq_objective(lp, None, 'mmi', 0.8, LM, 0.0)
    assert float((obj - post.log_z).abs().max()) <= 1e-9
    assert float((arc_grad - post.arc_log_post.exp()).abs().max()) <= 1e-9
    assert float((occ - post.frame_posteriors(24, 49)).abs().max()) <= 1e-6


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('key', [('unq', 4.0), ('fan',), ('mixed',)])
def test_repeatable_bits(key, monkeypatch):
    batch = device_case(key)[0]
    for criterion in cases.CRITERIA:
        first = launch(key, criterion, 0.5)
        assert same_bits(first, launch(key, criterion, 0.5))
        # one utterance per launch
        budget = 32 * int(np.diff(batch.node_off).max()) + 64          # the largest utterance alone
        chunks = batch._utterance_chunks(32, budget)
        assert len(chunks) > 1 or batch.num_utterances == 1
        split = launch(key, criterion, 0.5, workspace_bytes=budget)
        assert batch.launches == len(chunks)
        assert same_bits(first, split)
        for threads in (64, 128, 256):
            monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', threads)
            assert same_bits(first, launch(key, criterion, 0.5)), threads
        monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', 0)
    with pytest.raises(ValueError):
        launch(key, 'mmi', 0.0, workspace_bytes=64)


def test_refusals_before_launch():
    batch, _, lp_d, ref_d, lp, _ = device_case(('toy', 'a', 1.0, 2.0))
    with pytest.raises(ValueError):
        batch.seq_objective(lp_d[:, :, :2].contiguous(), ref_d)        # the graph reads class 2
    with pytest.raises(ValueError):
        batch.seq_objective(lp_d[:4].contiguous(), ref_d[:, :4].contiguous())   # an utterance has 5 frames
    with pytest.raises(ValueError):
        batch.seq_objective(lp_d, ref_d[:, :4])
    with pytest.raises(ValueError):
        batch.seq_objective(lp_d, ref_d.t())
    with pytest.raises(ValueError):
        batch.seq_objective(torch.from_numpy(np.nan_to_num(lp)), ref_d)         # CPU scores, device batch
    with pytest.raises(ValueError):
        batch.seq_objective(lp_d.double(), ref_d)
    with pytest.raises(ValueError):
        batch.seq_objective(lp_d, ref_d, criterion='mpe')
    with pytest.raises(ValueError):
        batch.seq_objective(lp_d, ref_d, boost=-1.0)
    # nothing faulted: the device still answers
    obj = batch.seq_objective(lp_d, ref_d)[0]
    assert torch.isfinite(obj).all()


def test_a_malformed_batch_is_refused():
    """tensors changed behind the constructor's checks: the kernel's own range checks answer, after its one launch.
    A bad graph arc (`arc`) is refused before any launch: seq_objective gathers the input labels by it first, and
    DeviceLatticeBatch.ilabel checks the range before it indexes (tests/test_lattice_launch.py holds that check on
    the CPU, where an unchecked gather would raise IndexError instead)."""
    lats, lp, ref = load(('toy', 'a', 1.0, 2.0))
    lp_d, ref_d = torch.from_numpy(lp).to(dev()), torch.from_numpy(ref).to(dev())
    turned = int(np.nonzero(lats[0].src != lats[0].dst)[0][0])
    for field, index, value in (('dst', 3, 10 ** 6), ('arc', 1, 10 ** 6), ('node_level', 0, 10 ** 6),
                                ('out_ptr', 2, 10 ** 6), ('level_node', 1, 10 ** 6), ('in_ptr', 2, 10 ** 6),
                                ('in_arc', 1, 10 ** 6), ('src', 3, 10 ** 6),
                                ('dst', turned, None)):  # None: the arc turned round, its level does not rise
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
        getattr(batch, field)[index] = batch.src[index] if value is None else value
        with pytest.raises(ValueError, match='inconsistent'):
            batch.seq_objective(lp_d, ref_d, 'mmi', None, LM, 0.0)
        assert batch.launches == (0 if field == 'arc' else 1)


def test_switch_takes_the_twin(monkeypatch):
    key = ('unq', 2.0)
    batch, _, lp_d, ref_d, _, _ = device_case(key)
    monkeypatch.setenv('ASR_LATTICE_TRAIN_NATIVE', '0')
    batch.launches = -1
    out = batch.seq_objective(lp_d, ref_d, 'smbr', None, LM, 0.5)
    assert batch.launches == -1 and all(x.is_cuda for x in out)
    assert same_bits([x.cpu().numpy() for x in out], twin(key, 'smbr', 0.5))
    monkeypatch.delenv('ASR_LATTICE_TRAIN_NATIVE')
    batch.seq_objective(lp_d, ref_d, 'smbr', None, LM, 0.5)
    assert batch.launches == 1


def test_autograd_function_on_the_device():
    key = ('unq', 2.0)
    batch, _, lp_d, ref_d, _, _ = device_case(key)
    w = torch.tensor([0.5, -1.0, 2.0, 0.25], device=dev())
    for criterion in cases.CRITERIA:
        x = lp_d.clone().requires_grad_()
        out = lattice_objective(x, batch, ref_d, criterion, 0.8, LM, 0.5)
        assert out.dtype == torch.float32 and out.is_cuda and out.skipped == 0
        (out * w).sum().backward()
        obj, _, occ = launch(key, criterion, 0.5, 0.8)
        assert (out.detach().cpu().numpy() == obj.astype(np.float32)).all()
        assert (x.grad == torch.from_numpy(occ).to(dev()) * (w * 0.8)[None, :, None]).all()


LABELS = [[3, 7, 7, 12, 5], [9, 2, 30, 4], [48, 1, 6], [11]]


@pytest.mark.parametrize('cls,boost', [(LatticeMMILoss, 0.0), (LatticeMMILoss, 0.5), (LatticeSMBRLoss, 0.0)])
def test_end_to_end_against_the_cpu_modules(cls, boost):
    """logits [24, 4, 49] -> log_softmax -> the loss, on the device and on CPU copies.  Tolerance: grad_atol of
    tests/test_lattice_gpu.py, the fp32 bound of the project's lattice losses against their CPU references."""
    logits = nbest_cases.unquantised_scores().clone()
    lens, lls = nbest_cases.UNQUANTISED_LENS, [len(r) for r in LABELS]
    flat = torch.tensor([v for r in LABELS for v in r])
    mod = cls(nbest_cases.bigram_graph(), beam=16.0, lattice_beam=4.0, acoustic_scale=0.9, lm_scale=LM, boost=boost)
    got = {}
    for where in ('cpu', dev()):
        x = logits.clone().to(where).requires_grad_()
        loss = mod(torch.log_softmax(x, -1), lens, flat, lls)
        assert loss.skipped == 0
        loss.backward()
        got[str(where)] = (float(loss), x.grad.cpu().numpy())
    (l_cpu, g_cpu), (l_gpu, g_gpu) = got['cpu'], got[str(dev())]
    # the fp32 part of both sides is the CTC numerator (and the log-softmax): its log-likelihoods set the scale
    atol = grad_atol(ctc_loglik(torch.log_softmax(logits, -1), flat, lens, lls).numpy())
    assert abs(l_gpu - l_cpu) <= RTOL_LOSS * max(1.0, abs(l_cpu)), (l_gpu, l_cpu)
    assert np.isfinite(g_gpu).all() and np.abs(g_gpu).max() > 0
    assert np.abs(g_gpu - g_cpu).max() <= atol, (float(np.abs(g_gpu - g_cpu).max()), atol)
