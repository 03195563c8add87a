"""Shared inputs of the WFST decoding tests (tests/test_wfst_decode.py on the CPU,
tests/test_wfst_decode_gpu.py on the GPU).  Everything sits on a 2^-8 grid with |lp| <= 32 and
T <= 64: every fp32 sum the search forms is then exact, so fp32 and the fp64 referee must agree
in every bit."""
import numpy as np

INF = float('inf')
GRID = 256.0

# (src, ilabel, olabel, weight, dst); C = 3 classes
TOY_A = dict(
    # an epsilon chain 0 -> 3 -> 4 -> 5 three deep with a negative weight, words on epsilon and
    # on emitting arcs, epsilon arcs into a final state
    arcs=[(0, 1, 0, 0.5, 1), (0, 2, 5, 1.25, 2), (0, 0, 7, 0.25, 3), (3, 0, 0, -0.75, 4),
          (4, 0, 8, 0.5, 5), (5, 1, 9, 0.0, 1), (5, 3, 0, 1.0, 6), (1, 1, 0, 0.25, 1),
          (1, 2, 6, 0.5, 2), (1, 0, 0, 1.5, 3), (2, 3, 0, 0.75, 0), (2, 2, 0, 0.25, 2),
          (2, 0, 4, 0.125, 6), (6, 1, 0, 0.5, 0), (6, 3, 3, 2.0, 6), (4, 2, 0, 0.375, 2)],
    final={2: 0.5, 5: 1.0, 6: 0.0}, states=7)
TOY_B = dict(
    # parallel arcs of equal cost with different words (the smaller arc index must win), an
    # epsilon arc that ties with an emitting arc into state 2, a final state behind an epsilon arc
    arcs=[(0, 1, 1, 0.5, 1), (0, 1, 2, 0.5, 1), (0, 2, 0, 0.5, 2), (1, 0, 3, 0.0, 2),
          (1, 1, 0, 1.0, 3), (2, 2, 4, 0.25, 3), (2, 1, 0, 0.5, 1), (3, 0, 0, 0.5, 4),
          (3, 1, 5, 0.0, 0), (4, 2, 0, 0.0, 4), (4, 1, 6, 0.25, 2), (0, 1, 0, 0.5, 2)],
    final={3: 1.0, 4: 0.25}, states=5)
TOY_C = dict(
    # eight states; the only final state needs at least three frames
    arcs=[(0, 1, 1, 0.25, 1), (0, 2, 0, 0.5, 2), (1, 2, 2, 0.5, 3), (2, 1, 0, 0.25, 3), (1, 0, 0, 0.125, 4),
          (4, 0, 3, -0.25, 5), (5, 0, 0, 0.5, 6), (6, 3, 4, 0.0, 3), (3, 3, 5, 0.75, 7), (3, 1, 0, 0.5, 3),
          (7, 2, 0, 0.25, 7), (7, 0, 6, 1.0, 2), (2, 3, 0, 1.5, 0)],
    final={7: 0.5}, states=8)
TOYS = dict(a=TOY_A, b=TOY_B, c=TOY_C)


def toy_graph(name):
    from att_speech.wfst_decode import DecodingGraph
    t = TOYS[name]
    src, il, ol, w, dst = [np.array(x) for x in zip(*t['arcs'])]
    final = np.full(t['states'], INF)
    for s, v in t['final'].items():
        final[s] = v
    return DecodingGraph(t['states'], 0, src, dst, il, ol, w, final)


def grid_scores(rng, T, B, C, lens=None, low=-32.0):
    """lp [T,B,C] on the grid in [low, 0]; frames beyond lens are NaN (they must never be read)"""
    lp = rng.integers(int(low * GRID), 1, size=(T, B, C)).astype(np.float32) / np.float32(GRID)
    if lens is not None:
        for b, n in enumerate(lens):
            lp[n:, b] = np.nan
    return lp


def random_graph(rng, N, C, arcs_per_state=4, eps_share=0.15, final_share=0.2, max_w=4.0, n_words=50):
    """A sparse random graph on the grid.  States fall into three classes by id % 3 and epsilon
    arcs lead from class k to class k + 1 only: acyclic, two epsilon ranks."""
    from att_speech.wfst_decode import DecodingGraph
    A = N * arcs_per_state
    src = rng.integers(0, N, size=A)
    dst = rng.integers(0, N, size=A)
    il = rng.integers(1, C + 1, size=A)
    eps = (rng.random(A) < eps_share) & (src % 3 < 2)
    up = (dst // 3) * 3 + (src % 3) + 1
    eps &= up < N
    dst[eps] = up[eps]
    il[eps] = 0
    ol = np.where(rng.random(A) < 0.3, rng.integers(1, n_words + 1, size=A), 0)
    w = rng.integers(-int(0.5 * GRID), int(max_w * GRID), size=A) / GRID
    final = np.where(rng.random(N) < final_share, rng.integers(0, int(2 * GRID), size=N) / GRID, INF)
    return DecodingGraph(N, 0, src, dst, il, ol, w, final)


FIELDS = ('alignment', 'cost', 'reached_final', 'num_active')


def assert_same(got, want, what=''):
    """every field equal; costs compared as numbers with == (fp32 against fp64 is exact on the grid)"""
    def arr(v):
        return v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)
    assert [list(w) for w in got['words']] == [list(w) for w in want['words']], what
    for k in FIELDS:
        g, w = arr(got[k]), arr(want[k])
        assert g.shape == w.shape, (what, k)
        assert (g.astype(np.float64) == w.astype(np.float64)).all(), (what, k, g, w)
