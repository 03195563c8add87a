"""asr_lattice_bestpath_f64 and asr_lattice_posterior_f64 (csrc/lattice_dp.hip) through
att_speech.lattice_dp: lattices that stay on the device, the sweep over scale pairs against
LatticeBatch.best_paths with == on words and on all three costs, and the posteriors against direct
summation over enumerated paths (tests/lattice_dp_referee.py) and against the numpy host path.

In every test nothing is redone on the host and the package raises no warning (the one overflow
case excepted, which expects exactly one).

lm_scale = 0: LatticeBatch.best_paths forms 0 * inf = NaN at every node that ends no path and so
returns ([], inf, inf, inf) for every utterance; the device reproduces those bits too.

Posterior tolerance (device against enumerator or host): 1e-9 absolute on log_z and on every
arc_log_post / node_log_post above -30, 1e-12 on the linear posterior below.  Both sides are fp64
logsumexp chains of depth at most 3 (T + 1) <= 200 over values of magnitude below 1e3, each step
good to a few ulp: about 200 * 4 * 1.1e-16 * 1e3 ~ 1e-10, and an order of magnitude is left for the
differing exp / log implementations."""
import warnings
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import lattice_dp_referee as DR
import wfst_lattice_referee as LR
from wfst_cases import INF, TOYS, grid_scores, random_graph, toy_graph

from att_speech import lattice_dp, wfst_lattice
from att_speech._native import lib
from att_speech.lattice_dp import DeviceLatticeBatch, decode_lattice_device
from att_speech.wfst_decode import DecodingGraph
from att_speech.wfst_lattice import Lattice, LatticeBatch, decode_lattice

pytestmark = pytest.mark.gpu

LENS = [5, 1, 3, 5]
LATTICE_BEAMS = (0.0, 2.0, INF)
SWEEP = [(1, 1), (0.5, 1), (0.1, 1), (0, 1), (1, 0), (None, 1)]
NONE = ([], INF, INF, INF)
TOL = 1e-9


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device('cuda:0')


@contextmanager
def quiet():
    """no warning from the package inside"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        yield
    ours = [str(w.message) for w in rec if 'att_speech' in (w.filename or '') or 'lattice' in str(w.message)]
    assert ours == [], ours


def device_batch(g, lp, lens, **kw):
    with quiet():
        batch, redone = decode_lattice_device(torch.from_numpy(lp).to(dev()), lens, g, **kw)
    assert redone == [] and batch.device.type == 'cuda'
    return batch


def host_best(batch, pairs):
    host = LatticeBatch(batch.lattices())
    with np.errstate(invalid='ignore'):                 # lm_scale = 0: 0 * inf on the host
        return [host.best_paths(sc, lm) for sc, lm in pairs]


def check_sweep(batch, pairs, **kw):
    with quiet():
        got = batch.best_paths([sc for sc, _ in pairs], [lm for _, lm in pairs], **kw)
    want = host_best(batch, pairs)
    assert len(got) == len(pairs)
    for k, pair in enumerate(pairs):
        for b in range(batch.num_utterances):
            assert got[k][b] == want[k][b], (pair, b, got[k][b], want[k][b])    # == on words and costs
    return got


def assert_log_close(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape and got.dtype == np.float64, what
    big = want > -30.0
    print(what, 'max |diff| above -30:', np.abs(got[big] - want[big]).max() if big.any() else 0.0)
    assert (np.abs(got[big] - want[big]) <= TOL).all(), what
    assert (np.abs(np.exp(got[~big]) - np.exp(want[~big])) <= 1e-12).all(), what
    assert ((got == -INF) == (want == -INF)).all(), what


def check_frames(post, lens, T, C):
    frames = post.frame_posteriors()
    assert frames.shape == (T, len(lens), C) and frames.dtype == torch.float32 and frames.is_cuda
    for b, n in enumerate(lens):
        assert float((frames[:n, b].sum(-1) - 1.0).abs().max()) < 1e-5, b
        assert bool((frames[n:, b] == 0).all()), b


def toy_inputs(name):
    return toy_graph(name), grid_scores(np.random.default_rng(len(name) + 3), 5, 4, 3, LENS, low=-4.0)


_SHARED = {}


def unquantised():
    """case 2: lp = log_softmax(N(0, 1)) on random_graph(600, 50); seed 0 picked on the host path so
    that the best words change along the sweep"""
    if 'u' not in _SHARED:
        rng = np.random.default_rng(0)
        g = random_graph(rng, 600, 50)
        lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((12, 3, 50)).astype(np.float32)), -1).numpy()
        _SHARED['u'] = (g, lp, [12, 7, 12], device_batch(g, lp, [12, 7, 12], beam=INF, lattice_beam=4.0))
    return _SHARED['u']


def large():
    """case 4: lattice_beam = 60 picked on the host path: 79 436 arcs and 60 280 nodes in utterance 0"""
    if 'l' not in _SHARED:
        rng = np.random.default_rng(70)
        g = random_graph(rng, 70000, 50, arcs_per_state=4)
        lens = [12, 7, 12]
        lp = grid_scores(rng, 12, 3, 50, lens)
        _SHARED['l'] = (g, lp, lens, device_batch(g, lp, lens, beam=INF, lattice_beam=60.0))
    return _SHARED['l']


@pytest.mark.parametrize('name', sorted(TOYS))
def test_toy_sweep(name):
    """(0, 1) makes every acoustic tie real; utterance 1 of toys b and c reaches no final state"""
    g, lp = toy_inputs(name)
    for lb in LATTICE_BEAMS:
        batch = device_batch(g, lp, LENS, beam=INF, lattice_beam=lb)
        got = check_sweep(batch, SWEEP)
        assert got[0] == got[5]                         # None: the scale of the search, 1
        assert all(r != NONE for r in got[0]) and all(r == NONE for r in got[4])
        for k in (0, 1):                                # and against the enumerator's own tie rule
            for b, lat in enumerate(batch.lattices()):
                assert got[k][b] == DR.best_path(lat, *SWEEP[k]), (name, lb, k, b)
    if name in 'bc':
        assert not batch.reached_final[1]


def test_unquantised_scores():
    """bit equality off the 2^-8 grid: the kernel's fp64 arithmetic is the host's, uncontracted"""
    g, lp, lens, batch = unquantised()
    scales = [round(1.0 - 0.1 * i, 1) for i in range(10)]
    got = check_sweep(batch, [(s, 1.0) for s in scales])
    assert any(got[i][b][0] != got[j][b][0] for b in range(3) for i in range(10) for j in range(i))
    assert any(c != round(c * 256) / 256 for _, c, _, _ in got[3])     # costs off the grid indeed


def test_ties_by_arc_index():
    """3000 arcs into one node, most at equal cost: the host takes the smallest graph arc index"""
    rng = np.random.default_rng(7)
    F, C = 3000, 5
    hub, sink, end = 0, F + 1, F + 2
    mid = np.arange(1, F + 1)
    src = np.concatenate([np.full(F, hub), mid, [sink, sink, hub, sink]])
    dst = np.concatenate([mid, np.full(F, sink), [hub, end, hub, sink]])
    il = np.concatenate([rng.integers(1, C + 1, F), rng.integers(1, 3, F), [1, 0, 2, 3]])
    ol = np.concatenate([rng.permutation(F) + 1, rng.permutation(F) + 5000, [0, 9001, 9002, 0]])
    w = np.concatenate([rng.integers(0, 2, F) / 4.0, np.zeros(F), [0.5, 0.25, 1.0, 0.75]])
    final = np.full(F + 3, INF)
    final[end] = 0.5
    final[5] = 0.0
    perm = rng.permutation(len(src))
    g = DecodingGraph(F + 3, 0, src[perm], dst[perm], il[perm], ol[perm], w[perm], final)
    lens = [4, 3]
    lp = -rng.integers(1, 3, size=(4, 2, C)).astype(np.float32)
    lp[3:, 1] = np.nan
    batch = device_batch(g, lp, lens, beam=INF, lattice_beam=0.5)
    in_degree = (batch.in_ptr[1:] - batch.in_ptr[:-1]).max()
    assert int(in_degree) > 500 and batch.num_arcs > 3000
    got = check_sweep(batch, [(1, 1), (0, 1)])
    assert all(len(words) >= 2 for words, _, _, _ in got[1])


def test_large_lattice():
    """more than 65 536 arcs and nodes in one lattice: no 16-bit index, nothing resident in LDS"""
    g, lp, lens, batch = large()
    arcs = np.diff(batch.arc_off)
    assert arcs.max() > 65536 and np.diff(batch.node_off).max() > 32768, arcs
    check_sweep(batch, [(1.0, 1.0), (0.5, 1.0), (0.2, 1.0)])
    with quiet():
        post = batch.posteriors()
    host = LatticeBatch(batch.lattices()).posteriors()
    assert_log_close(post.log_z, host.log_z, 'large log_z')
    check_frames(post, lens, 12, 50)


def test_many_levels():
    """64 frames x 3 ranks of levels beside a single frame"""
    g = toy_graph('c')
    lens = [64, 1]
    lp = grid_scores(np.random.default_rng(64), 64, 2, 3, lens, low=-4.0)
    batch = device_batch(g, lp, lens, beam=INF, lattice_beam=INF)
    levels = np.diff(batch.level_off)
    assert levels[0] > 3 * 64 and levels[1] <= 6, levels
    got = check_sweep(batch, SWEEP)
    assert len(got[0][0][0]) > 10
    with quiet():
        post = batch.posteriors()
    assert_log_close(post.log_z, LatticeBatch(batch.lattices()).posteriors().log_z, 'levels log_z')
    check_frames(post, lens, 64, 3)


def test_empty_and_partial():
    g = toy_graph('c')                                  # its final state is at least three frames away
    lens = [1, 5, 2]
    lp = grid_scores(np.random.default_rng(4), 5, 3, 3, lens, low=-4.0)
    gone = device_batch(g, lp, lens, beam=INF, lattice_beam=2.0, allow_partial=False)
    assert np.diff(gone.node_off).tolist()[0] == 0 and np.diff(gone.node_off)[1] > 0
    partial = device_batch(g, lp, lens, beam=INF, lattice_beam=2.0, allow_partial=True)
    assert not partial.reached_final[0] and np.diff(partial.node_off)[0] > 0
    # one batch with an empty, a complete and a partial lattice, uploaded from the host
    mixed = [gone.lattices()[0], gone.lattices()[1], partial.lattices()[2]]
    with quiet():
        uploaded = DeviceLatticeBatch.from_lattices(mixed, dev())
    for batch, empty in ((gone, [0, 2]), (uploaded, [0]), (partial, [])):
        got = check_sweep(batch, SWEEP[:3])
        with quiet():
            post = batch.posteriors()
        log_z = post.log_z.cpu().numpy()
        for b in range(3):
            assert (got[0][b] == NONE) == (b in empty)
            assert (log_z[b] == -INF) == (b in empty)
        for b, lat in enumerate(batch.lattices()):
            assert b in empty or abs(log_z[b] - DR.posteriors(lat)[0]) <= TOL
    back = uploaded.lattices()
    for a, b in zip(back, mixed):
        assert a.cost == b.cost and a.reached_final == b.reached_final and a.num_frames == b.num_frames
        for f in Lattice.FIELDS:
            assert (getattr(a, f) == getattr(b, f)).all()


def test_chunking():
    """a workspace that holds neither all pairs nor all utterances: several launches, same results"""
    g, lp, lens, batch = unquantised()
    pairs = [(round(1.0 - 0.1 * i, 1), 1.0) for i in range(10)]
    whole = check_sweep(batch, pairs)
    assert batch.launches == 1
    nodes = np.diff(batch.node_off)
    by_pairs = check_sweep(batch, pairs, workspace_bytes=12 * 3 * batch.num_nodes + 64)
    assert batch.launches == 4                          # three pairs a launch
    by_both = check_sweep(batch, pairs, workspace_bytes=12 * int(nodes.max()) + 64)
    assert batch.launches >= 20                         # one pair, and not all utterances, a launch
    assert whole == by_pairs == by_both
    budget = 16 * int(nodes.max()) + 64
    with quiet():
        a = batch.posteriors(0.5)
        assert batch.launches == 1
        b = batch.posteriors(0.5, workspace_bytes=budget)
    assert batch.launches == len(batch._utterance_chunks(16, budget)) > 1
    assert torch.equal(a.arc_log_post, b.arc_log_post) and torch.equal(a.log_z, b.log_z)
    with pytest.raises(ValueError, match='workspace_bytes'):
        batch.best_paths(1.0, workspace_bytes=12 * int(nodes.max()))


def _as_dict(lat):
    d = {f: getattr(lat, f) for f in Lattice.FIELDS}
    d.update(cost=lat.cost, reached_final=lat.reached_final)
    return d


@pytest.mark.parametrize('name', sorted(TOYS))
def test_device_batch_equals_decode_lattice(name):
    g, lp = toy_inputs(name)
    for scale in (1.0, 0.5):
        for lb in LATTICE_BEAMS:
            kw = dict(beam=INF, lattice_beam=lb, acoustic_scale=scale)
            want, redone = decode_lattice(torch.from_numpy(lp).to(dev()), LENS, g, **kw)
            assert redone == []
            got = device_batch(g, lp, LENS, **kw).lattices()
            assert len(got) == len(want)
            for a, b in zip(got, want):
                LR.assert_same(a, _as_dict(b), (name, kw))
                assert (a.num_frames, a.acoustic_scale) == (b.num_frames, b.acoustic_scale)
                assert all(getattr(a, f).dtype == getattr(b, f).dtype for f in Lattice.FIELDS)


def test_overflow_is_redone_into_its_place(monkeypatch):
    """capacities that utterance 1 alone outgrows (its token list): redone on the host with the one
    warning, and the redone lattice sits in its place on the device"""
    rng = np.random.default_rng(12)
    g = random_graph(rng, 300, 11)
    lens = [3, 16, 3]
    lp = grid_scores(rng, 16, 3, 11, lens)
    kw = dict(beam=INF, lattice_beam=2.0)
    want = decode_lattice(torch.from_numpy(np.nan_to_num(lp)), lens, g, **kw)[0]       # the host path
    monkeypatch.setattr(wfst_lattice, 'plan_workspace',
                        lambda N, T, B, budget, A=None: (B, 150, 17 * 300, 17 * 300, 17 * 1200))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        batch, redone = decode_lattice_device(torch.from_numpy(lp).to(dev()), lens, g, **kw)
    msgs = [str(w.message) for w in rec if 'decode_lattice' in str(w.message)]
    assert len(msgs) == 1 and 'list' in msgs[0] and redone == [1]
    assert batch.time.is_cuda and np.diff(batch.node_off)[1] == want[1].num_nodes > 0
    for a, b in zip(batch.lattices(), want):
        LR.assert_same(a, _as_dict(b))
    check_sweep(batch, [(1, 1), (0.5, 1)])


@pytest.mark.parametrize('name', sorted(TOYS))
def test_posteriors_against_the_enumerator(name):
    g, lp = toy_inputs(name)
    for lb in LATTICE_BEAMS:
        batch = device_batch(g, lp, LENS, beam=INF, lattice_beam=lb)
        lats = batch.lattices()
        for sc, lm in ((1.0, 1.0), (0.5, 1.0), (1.0, 0.0)):
            with quiet():
                post = batch.posteriors(sc, lm)
                again = batch.posteriors(sc, lm)
            assert post.arc_log_post.is_cuda and post.arc_log_post.dtype == torch.float64
            for x, y in ((post.log_z, again.log_z), (post.arc_log_post, again.arc_log_post),
                         (post.node_log_post, again.node_log_post)):
                assert torch.equal(x, y)                # two runs, the same bits
            a0 = n0 = 0
            for b, lat in enumerate(lats):
                log_z, arcs, nodes = DR.posteriors(lat, sc, lm)
                what = (name, lb, sc, lm, b)
                assert_log_close(post.log_z[b:b + 1], [log_z], what)
                assert_log_close(post.arc_log_post[a0:a0 + lat.num_arcs], arcs, what)
                assert_log_close(post.node_log_post[n0:n0 + lat.num_nodes], nodes, what)
                a0, n0 = a0 + lat.num_arcs, n0 + lat.num_nodes
        check_frames(batch.posteriors(), LENS, 5, 3)
    words = batch.posteriors().word_posteriors(window=0)
    want = LatticeBatch(lats).posteriors().word_posteriors(window=0)
    assert [[(w, t) for w, t, _ in row] for row in words] == [[(w, t) for w, t, _ in row] for row in want]
    assert all(abs(p - q) < 1e-9 for r, s in zip(words, want) for (_, _, p), (_, _, q) in zip(r, s))


@pytest.mark.parametrize('case', ['unquantised', 'large'])
def test_posteriors_against_the_host_path(case):
    g, lp, lens, batch = unquantised() if case == 'unquantised' else large()
    host = LatticeBatch(batch.lattices())
    for sc in (None, 0.5):
        with quiet():
            post = batch.posteriors(sc)
            again = batch.posteriors(sc)
        want = host.posteriors(sc)
        assert_log_close(post.log_z, want.log_z, (case, sc, 'log_z'))
        assert_log_close(post.arc_log_post, want.arc_log_post, (case, sc, 'arcs'))
        assert_log_close(post.node_log_post, want.node_log_post, (case, sc, 'nodes'))
        assert torch.equal(post.arc_log_post, again.arc_log_post) and torch.equal(post.log_z, again.log_z)
        assert torch.equal(post.node_log_post, again.node_log_post)
        check_frames(post, lens, 12, 50)


def test_env_switch(monkeypatch):
    g, lp, lens, batch = unquantised()
    pairs = [(1.0, 1.0), (0.3, 1.0), (None, 2.0)]
    native = check_sweep(batch, pairs)
    calls = []
    real = LatticeBatch.best_paths
    monkeypatch.setattr(LatticeBatch, 'best_paths', lambda self, *a, **k: calls.append(a) or real(self, *a, **k))
    monkeypatch.setenv('ASR_LATTICE_DP_NATIVE', '0')
    batch.launches = 0
    with quiet():
        host = batch.best_paths([sc for sc, _ in pairs], [lm for _, lm in pairs])
        post = batch.posteriors(0.5)
    assert len(calls) == 3 and batch.launches == 0 and host == native
    monkeypatch.delenv('ASR_LATTICE_DP_NATIVE')
    assert_log_close(batch.posteriors(0.5).arc_log_post, post.arc_log_post.cpu().numpy(), 'env')


def test_a_malformed_batch_is_refused():
    """tensors changed behind the constructor's checks: the kernels' own range checks answer.  best_paths never
    reads out_ptr (it walks the in-arcs only), so that field is posteriors' alone.  Both operations count their one
    launch; the message is the one raised on the status words the kernel wrote."""
    import nbest_cases as NC
    lats, _ = NC.toy_lattices('a', 1.0, 2.0)
    turned = int(np.nonzero(lats[0].src != lats[0].dst)[0][0])
    fields = (('dst', 3, 10 ** 6), ('arc', 1, 10 ** 6), ('node_level', 0, 10 ** 6), ('out_ptr', 2, 10 ** 6),
              ('level_node', 1, 10 ** 6), ('in_ptr', 2, 10 ** 6), ('in_arc', 1, 10 ** 6), ('src', 3, 10 ** 6),
              ('dst', turned, None))                    # None: the arc turned round, its level does not rise
    for field, index, value in fields:
        for op, entry in (('best_paths', 'asr_lattice_bestpath_f64'), ('posteriors', 'asr_lattice_posterior_f64')):
            if (op, field) == ('best_paths', 'out_ptr'):
                continue
            with quiet():
                batch = DeviceLatticeBatch.from_lattices(lats, dev())
            getattr(batch, field)[index] = batch.src[index] if value is None else value
            with pytest.raises(ValueError, match=entry + '.*inconsistent'):
                getattr(batch, op)()
            assert batch.launches == 1


def test_the_entry_points_are_exported():
    L = lib()
    assert L.asr_lattice_bestpath_supported(1000, 5000, 300) == 1
    assert L.asr_lattice_bestpath_supported(2 ** 31, 5000, 300) == 0
    assert L.asr_lattice_posterior_supported(1000, 5000, 300) == 1
    assert L.asr_lattice_bestpath_workspace_bytes(1000, 10) >= 12 * 1000 * 10
    assert L.asr_lattice_posterior_workspace_bytes(1000) >= 16 * 1000
    assert L.asr_abi_version() == 24
    assert lattice_dp.THREADS_PER_WORKGROUP == 0
