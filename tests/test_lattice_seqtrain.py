"""Sequence-discriminative training on lattices, on the CPU: the numpy twin
(LatticeBatch.seq_objective) against brute-force enumeration of every path and against the existing
posteriors, the autograd function and the loss modules on CPU tensors, and the C ABI without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import nbest_cases
import seqtrain_cases as cases
from conftest import ROOT  # noqa: F401

from att_speech import _native
from att_speech.lattice_dp import DeviceLatticeBatch
from att_speech.lattice_train import lattice_objective
from att_speech.modules.sequence_losses import LatticeMMILoss, LatticeSMBRLoss, ctc_loglik
from att_speech.wfst_lattice import LatticeBatch

INF = float('inf')
LM = 1.25


def close(got, want, what):
    """within 1e-9 max(1, |value|), the bound of the issue; infinities must agree"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all() and (got[~fin] == want[~fin]).all(), what
    err = np.abs(got[fin] - want[fin]) - 1e-9 * np.maximum(1.0, np.abs(want[fin]))
    assert (err <= 0).all(), (what, float(err.max()))


def check_against_brute_force(lats, lp, ref, scale):
    hb = LatticeBatch(lats)
    T, B, C = lp.shape
    s = np.array([l.acoustic_scale if scale is None else scale for l in lats])
    counts = None
    for criterion in cases.CRITERIA:
        for boost in cases.BOOSTS:
            what = (criterion, boost, scale)
            obj, arc_grad, occ = hb.seq_objective(lp.astype(np.float64), ref, criterion, scale, LM, boost)
            want_obj, want_grad, counts = cases.brute_force(lats, lp, ref, criterion, scale, LM, boost)
            close(obj, want_obj, what)
            sums = cases.arc_sums(cases.host_arrays(hb), arc_grad, T, B, C)
            close(sums * s[None, :, None], want_grad, what)
            assert occ.dtype == np.float32 and (occ == sums.astype(np.float32)).all(), what
            if criterion == 'smbr':             # a single path: every arc is as accurate as the average
                single = np.isin(hb.n_utt[hb.src], np.nonzero(np.array(counts) == 1)[0])
                assert (arc_grad[single] == 0.0).all(), what
    return counts


@pytest.mark.parametrize('name,scale,lb', nbest_cases.sweep())
def test_twin_against_brute_force_on_the_toy_sweep(name, scale, lb):
    lats, lp, ref = cases.toy_case(name, scale, lb)
    counts = check_against_brute_force(lats, lp, ref, None if lb != 1.0 else 0.75)
    assert min(counts) >= 1


def test_the_toy_sweep_is_what_the_tests_assume():
    """120 lattices, none empty, 13 with a single path, at most 1594 complete paths: all enumerable"""
    counts = []
    for name, scale, lb in nbest_cases.sweep():
        counts += [len(cases.complete_paths(lat)[0]) for lat in cases.toy_case(name, scale, lb)[0]]
    assert len(counts) == 120 and min(counts) >= 1
    assert sum(1 for c in counts if c == 1) == 13 and max(counts) == 1594


def test_twin_against_brute_force_on_the_unquantised_bigram():
    lats, lp, ref = cases.unquantised_case(2.0)
    assert check_against_brute_force(lats, lp, ref, None) == [4928, 2336, 96, 2]
    assert (lp != nbest_cases.unquantised_scores().numpy()).all()      # the live scores are not the stored ones


def test_twin_without_a_reference():
    lats, lp, _ = cases.toy_case('b', 1.0, 4.0)
    hb = LatticeBatch(lats)
    for criterion in cases.CRITERIA:
        obj, arc_grad, occ = hb.seq_objective(lp.astype(np.float64), None, criterion, None, LM, 0.5)
        want_obj, want_grad, _ = cases.brute_force(lats, lp, None, criterion, None, LM, 0.5)
        close(obj, want_obj, criterion)
        close(cases.arc_sums(cases.host_arrays(hb), arc_grad, *lp.shape), want_grad, criterion)
        if criterion == 'smbr':                 # no accuracies: nothing to expect
            assert (obj == 0).all() and (arc_grad == 0).all() and (occ == 0).all()


def _posterior_inputs():
    out = [(cases.toy_case(*pt)[0], nbest_cases.toy_inputs(pt[0])[1]) for pt in nbest_cases.sweep()]
    return out + [(nbest_cases.unquantised_lattices(lb), nbest_cases.unquantised_scores().numpy())
                  for lb in nbest_cases.UNQUANTISED_BEAMS]


def test_twin_against_the_posteriors_on_the_decode_scores():
    """with the tensor the lattice was decoded from, no reference and no boost, 'mmi' is posteriors()"""
    for lats, lp in _posterior_inputs():
        hb = LatticeBatch(lats)
        for scale, lm in ((None, 1.0), (0.6, LM)):
            post = hb.posteriors(scale, lm)
            obj, arc_grad, occ = hb.seq_objective(lp, None, 'mmi', scale, lm, 0.0)
            assert np.abs(obj - post.log_z).max() <= 1e-9
            assert np.abs(arc_grad - np.exp(post.arc_log_post)).max() <= 1e-9
            want = post.frame_posteriors(*lp.shape[::2]).numpy()
            assert occ.shape == want.shape
            ulp = np.spacing(np.maximum(np.abs(want), np.abs(occ)).astype(np.float32))
            assert (np.abs(occ.astype(np.float64) - want) <= ulp).all()


def test_twin_refuses_what_it_cannot_index():
    lats, lp, ref = cases.toy_case('a', 1.0, 2.0)
    hb = LatticeBatch(lats)
    with pytest.raises(ValueError):
        hb.seq_objective(lp[:, :, :2], ref)                     # the graph reads class 2
    with pytest.raises(ValueError):
        hb.seq_objective(lp[:4], ref[:, :4])                    # an utterance has 5 frames
    with pytest.raises(ValueError):
        hb.seq_objective(lp, ref[:, :4])
    with pytest.raises(ValueError):
        hb.seq_objective(lp, ref, criterion='mpe')
    with pytest.raises(ValueError):
        hb.seq_objective(lp, ref, boost=-0.5)


def test_no_path_and_partial_utterances():
    lats, lp, ref = cases.mixed_case()
    hb = LatticeBatch(lats)
    mmi = hb.seq_objective(lp, ref, 'mmi', None, LM, 0.5)
    smbr = hb.seq_objective(lp, ref, 'smbr', None, LM, 0.5)
    assert mmi[0][1] == -INF and smbr[0][1] == 0.0 and np.isfinite(np.delete(mmi[0], 1)).all()
    assert (mmi[2][:, 1] == 0).all() and (smbr[2][:, 1] == 0).all()
    for criterion, got in (('mmi', mmi), ('smbr', smbr)):
        want_obj, want_grad, counts = cases.brute_force(lats, lp, ref, criterion, None, LM, 0.5)
        assert counts[1] == 0 and min(counts[0], counts[2], counts[3]) > 1
        close(got[0], want_obj, criterion)
        close(cases.arc_sums(cases.host_arrays(hb), got[1], *lp.shape), want_grad, criterion)
    # without a final state reached, every node of the last frame ends a path: more paths than before
    full = cases.toy_case('a', 1.0, 2.0)[0][2]
    assert len(cases.complete_paths(lats[2])[0]) >= len(cases.complete_paths(full)[0])


# ---- the autograd function and the modules on CPU tensors ------------------------------------------

def test_autograd_function_on_cpu_tensors():
    lats, lp, ref = cases.unquantised_case(2.0)
    batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
    hb = LatticeBatch(lats)
    w = torch.tensor([0.5, -1.0, 2.0, 0.25])
    rng = np.random.default_rng(3)
    for criterion in cases.CRITERIA:
        for scale in (None, 0.8):
            x = torch.from_numpy(lp).requires_grad_()
            out = lattice_objective(x, batch, torch.from_numpy(ref), criterion, scale, LM, 0.5)
            assert out.dtype == torch.float32 and out.shape == (4,) and out.skipped == 0
            obj, _, occ = hb.seq_objective(lp, ref, criterion, scale, LM, 0.5)
            assert (out.detach().numpy() == obj.astype(np.float32)).all()
            (out * w).sum().backward()
            sc = 1.0 if scale is None else scale
            want = torch.from_numpy(occ) * (w * sc)[None, :, None]
            assert (x.grad == want).all()
            # and the occupancies are the derivative: a central difference of the twin in fp64
            d = rng.standard_normal(lp.shape)
            eps = 1e-5
            hi = hb.seq_objective(lp.astype(np.float64) + eps * d, ref, criterion, scale, LM, 0.5)[0]
            lo = hb.seq_objective(lp.astype(np.float64) - eps * d, ref, criterion, scale, LM, 0.5)[0]
            slope = (sc * occ.astype(np.float64) * d).sum((0, 2))
            assert np.abs((hi - lo) / (2 * eps) - slope).max() <= 1e-5 * max(1.0, np.abs(slope).max())


def test_autograd_function_skips_utterances_without_a_path():
    lats, lp, ref = cases.mixed_case()
    batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
    x = torch.from_numpy(np.nan_to_num(lp)).requires_grad_()
    for criterion in cases.CRITERIA:
        out = lattice_objective(x, batch, torch.from_numpy(ref), criterion, lm_scale=LM)
        assert out.skipped == 1 and out.has_path.tolist() == [True, False, True, True]
        assert float(out.detach()[1]) == 0.0 and torch.isfinite(out).all()
        x.grad = None
        out.sum().backward()
        assert torch.isfinite(x.grad).all() and (x.grad[:, 1] == 0).all() and (x.grad != 0).any()
    with pytest.raises(TypeError):
        lattice_objective(x, LatticeBatch(lats))


LABELS = [[3, 7, 7, 12, 5], [9, 2, 30, 4], [48, 1, 6], [11]]


def _module_inputs():
    logits = nbest_cases.unquantised_scores().clone()
    flat = torch.tensor([v for row in LABELS for v in row])
    return logits, nbest_cases.UNQUANTISED_LENS, flat, [len(r) for r in LABELS]


def test_mmi_module_is_the_hand_assembled_loss():
    logits, lens, flat, lls = _module_inputs()
    g = nbest_cases.bigram_graph()
    for boost in (0.0, 0.5):
        mod = LatticeMMILoss(g, beam=16.0, lattice_beam=2.0, acoustic_scale=0.9, lm_scale=LM, boost=boost)
        x = logits.clone().requires_grad_()
        lp = torch.log_softmax(x, -1)
        loss = mod(lp, lens, flat, lls)
        assert loss.skipped == mod.skipped == 0
        batch = mod.decode(lp, lens)
        ref = None
        if boost:
            from att_speech.modules.ctc_losses import ctc_viterbi_align_batch
            ref = ctc_viterbi_align_batch(lp.detach(), flat, lens, lls, num_symbols=49).frames
        log_z, _, occ = LatticeBatch(batch.lattices()).seq_objective(lp.detach().numpy(), ref, 'mmi', 0.9, LM, boost)
        num = ctc_loglik(lp.detach(), flat, lens, lls).double().numpy()
        want = -(0.9 * num - log_z).sum()
        assert abs(float(loss) - want) <= 1e-5 * abs(want)
        # passing the lattices in changes nothing
        again = mod(lp, lens, flat, lls, lattices=batch)
        assert float(again) == float(loss)
        loss.backward()
        assert torch.isfinite(x.grad).all() and (x.grad != 0).any()
        # the denominator's part of the gradient with respect to log_probs is sc occ
        y = lp.detach().clone().requires_grad_()
        mod(y, lens, flat, lls, lattices=batch).backward()
        z = lp.detach().clone().requires_grad_()
        (-0.9 * ctc_loglik(z, flat, lens, lls).sum()).backward()
        assert np.abs((y.grad - z.grad).numpy() - 0.9 * occ).max() <= 1e-6


def test_smbr_of_a_single_path_has_exactly_zero_gradient():
    logits, lens, flat, lls = _module_inputs()
    mod = LatticeSMBRLoss(nbest_cases.bigram_graph(), beam=16.0, lattice_beam=0.0, boost=0.5)
    x = logits.clone().requires_grad_()
    lp = torch.log_softmax(x, -1)
    batch = mod.decode(lp, lens)
    assert [len(cases.complete_paths(lat)[0]) for lat in batch.lattices()] == [1, 1, 1, 1]
    loss = mod(lp, lens, flat, lls, lattices=batch)
    loss.backward()
    assert loss.skipped == 0 and (x.grad == 0).all()
    # the loss itself is minus the number of frames on which the best path agrees with the alignment
    assert float(loss) == -round(-float(loss)) and -24 - 17 - 9 - 1 <= float(loss) <= 0


def test_smbr_module_against_the_twin():
    logits, lens, flat, lls = _module_inputs()
    mod = LatticeSMBRLoss(nbest_cases.bigram_graph(), beam=16.0, lattice_beam=2.0, acoustic_scale=0.9, lm_scale=LM)
    x = logits.clone().requires_grad_()
    lp = torch.log_softmax(x, -1)
    batch = mod.decode(lp, lens)
    loss = mod(lp, lens, flat, lls, lattices=batch)
    from att_speech.modules.ctc_losses import ctc_viterbi_align_batch
    ref = ctc_viterbi_align_batch(lp.detach(), flat, lens, lls, num_symbols=49).frames
    obj, _, occ = LatticeBatch(batch.lattices()).seq_objective(lp.detach().numpy(), ref, 'smbr', 0.9, LM, 0.0)
    assert abs(float(loss) + obj.sum()) <= 1e-5 * max(1.0, abs(obj.sum()))
    y = lp.detach().clone().requires_grad_()
    mod(y, lens, flat, lls, lattices=batch).backward()
    assert (y.grad.numpy() == -np.float32(0.9) * occ).all()


def test_modules_count_what_they_skip():
    lats, lp, _ = cases.mixed_case()
    batch = DeviceLatticeBatch.from_lattices(lats, 'cpu')
    x = torch.from_numpy(np.nan_to_num(lp)).requires_grad_()
    lens = nbest_cases.LENS                                     # [5, 1, 3, 5]
    rows = [[1, 2], [1], [2], [1, 1, 2, 2]]                     # the last needs 6 frames and has 5
    flat, lls = torch.tensor([v for r in rows for v in r]), [len(r) for r in rows]
    for mod in (LatticeMMILoss(batch.graph, boost=0.5), LatticeSMBRLoss(batch.graph)):
        loss = mod(x, lens, flat, lls, lattices=batch)
        assert loss.skipped == mod.skipped == 2 and bool(torch.isfinite(loss))
        x.grad = None
        loss.backward()
        assert torch.isfinite(x.grad).all()
        assert (x.grad[:, 1] == 0).all() and (x.grad[:, 3] == 0).all() and (x.grad[:, 0] != 0).any()
    with pytest.raises(TypeError):
        LatticeMMILoss(batch.graph)(x, lens, flat, lls, lattices=lats)
    with pytest.raises(ValueError):
        LatticeMMILoss(batch.graph, boost=-1.0)


# ---- the C ABI without a GPU ----------------------------------------------------------------------------

def _abi_call(L, criterion=0, boost=0.0, nulls=False, b_count=0):
    """asr_lattice_seqtrain_f64 on an empty batch of one utterance held in host memory: nothing is launched"""
    off = np.zeros(2, np.int64)
    one = np.zeros(1, np.int32)
    f = np.zeros(1, np.float32)
    d = np.zeros(1, np.float64)
    keep = [off, one, f, d]
    h = lambda a: None if nulls else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    head = (0, 0, 0, h(off), h(off), h(off), h(off), h(off), h(off), h(one), h(one), h(one), h(one), h(one),
            h(off), h(f), h(one), h(one), h(one), h(one), h(one), h(one), h(one), h(d))
    tail = (1, 0, h(f), h(one), h(f), 0, 0)
    code = L.asr_lattice_seqtrain_f64(1, 0, b_count, *head, float('nan'), 1.0, *tail, h(one), h(f), 1, 1, None,
                                      criterion, boost, 0, 0, h(one), h(one), h(off), h(off), h(d), h(d), h(f),
                                      h(one), None, 0, None)
    del keep
    return code


def test_argument_checks_need_no_gpu():
    L = _native.lib()
    assert L.asr_abi_version() == 24 == _native.ABI_VERSION
    for name in ('asr_lattice_seqtrain_supported', 'asr_lattice_seqtrain_workspace_bytes',
                 'asr_lattice_seqtrain_f64'):
        assert name in _native._SIGNATURES
    assert _abi_call(L) == _native.ASR_OK                      # no utterance to serve: nothing to launch
    assert _abi_call(L, nulls=True) == _native.ASR_EINVAL
    assert _abi_call(L, b_count=1) == _native.ASR_EINVAL       # an utterance, but no workspace
    for criterion in (-1, 2, 7):
        assert _abi_call(L, criterion=criterion) == _native.ASR_EINVAL
    assert _abi_call(L, criterion=1) == _native.ASR_OK
    for boost in (-0.5, float('nan'), INF):
        assert _abi_call(L, boost=boost) == _native.ASR_EINVAL
    assert _abi_call(L, boost=0.5) == _native.ASR_OK
    for n in (0, 1, 7, 1000):
        assert L.asr_lattice_seqtrain_workspace_bytes(n) >= 32 * n
    assert L.asr_lattice_seqtrain_workspace_bytes(-1) == 0
    assert L.asr_lattice_seqtrain_supported(10, 20, 5) == 1
    assert L.asr_lattice_seqtrain_supported(2 ** 31, 20, 5) == 0
    header = open(ROOT + '/include/asr_amd.h').read()
    assert 'asr_lattice_seqtrain_f64(' in header and 'Additions: the ABI version stays 24' in header
