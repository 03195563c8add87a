"""Lattices that stay on the device, and the two dynamic programmes run over them there.

`decode_lattice_device` is att_speech.wfst_lattice.decode_lattice without the copy to the host: the
same launch, the same canonical sort on the device, and a `DeviceLatticeBatch` instead of a list of
`Lattice`.  The batch re-ranks itself under any number of (acoustic scale, LM scale) pairs in one
launch (`best_paths`: the recipe's acoustic-scale sweep, egs/wsj/ctc_kaldi_decode.sh:160-163, as one
search plus one sweep) and computes arc, node, frame and word posteriors (`posteriors`:
lattice-to-post).  DESIGN.md section 4.21.  `nbest` / `sentences` list its n cheapest distinct word
sequences, the hand-over to AttentionDecoderTCN.score_sentences, in one launch (section 4.22).  `mbr`
decodes it by minimum Bayes risk (the word sequence of the least expected word edit distance, with
per-word confidences and the confusion network) and `expected_errors` scores given sentences by that
distance, all iterations in one launch of asr_lattice_mbr_f64 (section 4.23).  `oracle` finds the path nearest
to a reference in word edit distance (lattice-oracle) in one launch of asr_lattice_oracle_i32 (section 4.25),
and `depth` is lattice-depth.  `seq_objective` is the training side: the lattice MMI / boosted MMI denominator and
the sMBR objective from the live log_probs, with the occupancies as a [T, B, C] tensor, in one launch of
asr_lattice_seqtrain_f64 (csrc/lattice_train.hip, section 4.26; att_speech.lattice_train wraps it in autograd).

A batch on a GPU runs the six entry points asr_lattice_bestpath_f64, asr_lattice_posterior_f64, asr_lattice_nbest_f64,
asr_lattice_mbr_f64, asr_lattice_oracle_i32 and asr_lattice_seqtrain_f64, all through one chunked launch
(DeviceLatticeBatch._launch); a batch of CPU tensors, or ASR_LATTICE_<NAME>_NATIVE=0 (DP for
best_paths and posteriors, NBEST, MBR, ORACLE, TRAIN; read per call), the host path: LatticeBatch of
att_speech.wfst_lattice, which gives the same bits for best paths, n-best lists and the oracle, and the same
posteriors, MBR results and training statistics within rounding.
"""
import ctypes
import os
import warnings

import numpy as np
import torch

from att_speech import _native
from att_speech.wfst_decode import DEFAULT_WORKSPACE_BYTES
from att_speech.wfst_lattice import (INF, MBR_NONE, ORACLE_NONE, OVERFLOW_NAMES, Lattice, LatticeBatch,
                                     LatticePosteriors, MBRResult, OracleResult, _decode_device, _oracle_references,
                                     _order, _validate, decode_lattice_host, mbr_sausage, nbest_lists)

THREADS_PER_WORKGROUP = 0       # 0: the kernels' default (64; nbest, mbr and oracle: 256); 64 / 128 / 256 for timing runs
NBEST_DEVICE_MAX = 64           # ASR_LATTICE_NBEST_MAX of include/asr_amd.h: a list entry per lane of a wave
MBR_DEVICE_MAX_WORDS = 255      # ASR_LATTICE_MBR_MAX_WORDS: the longest hypothesis asr_lattice_mbr_f64 has columns for
ORACLE_DEVICE_MAX_WORDS = 1023  # ASR_LATTICE_ORACLE_MAX_WORDS: the longest reference asr_lattice_oracle_i32 has columns for
MBR_SAUSAGE_ENTRIES = 0         # sausage entries an utterance in mbr's buffer; 0: per slot a word of the graph each, at most 64


def _h(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _scale_list(v):
    if v is None or isinstance(v, (int, float, np.floating, np.integer)):
        return [v], True
    return list(v), False


class DeviceLatticeBatch(object):
    """The lattices of B utterances over one DecodingGraph as tensors on one device, in the canonical
    form of wfst_lattice.Lattice, utterance after utterance:

      time, state [N] int32, alpha, beta [N] float32        nodes by (utterance, time, state)
      src, dst [A] int32 (node indices within the utterance), arc [A] int64, lp [A] float32
                                                             arcs by (utterance, src, graph arc)
      node_off, arc_off [B+1] int64 (numpy, and *_d on the device), num_frames [B], reached_final [B],
      cost [B] float32, acoustic_scale [B] float64 (numpy: per utterance, the scale of its search)

    and the level structure the dynamic programmes walk, built once with torch ops on the device: a
    node's level is (time, graph.rank[state]) and every arc rises in level;

      node_level [N], level_ptr [L+1], level_node [N], level_off [B+1]   the nodes level by level
      in_ptr [N+1], in_arc [A]                                           the in-arcs of every node
      out_ptr [N+1]                                                      its out-arcs: a range of arcs

    Malformed arrays (an end point outside the utterance, a level that does not rise, arcs not sorted
    by source) raise ValueError here, before any kernel sees them."""

    def __init__(self, graph, device, time, state, alpha, beta, src, dst, arc, lp, node_count, arc_count,
                 num_frames, reached_final, cost, acoustic_scale, max_frames=None, num_classes=None,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        self.graph, self.device = graph, torch.device(device)
        dev = self.device
        self.time, self.state = time.to(dev, torch.int32), state.to(dev, torch.int32)
        self.alpha, self.beta = alpha.to(dev, torch.float32), beta.to(dev, torch.float32)
        self.src, self.dst = src.to(dev, torch.int32), dst.to(dev, torch.int32)
        self.arc, self.lp = arc.to(dev, torch.int64), lp.to(dev, torch.float32)
        node_count = np.asarray(node_count, np.int64).reshape(-1)
        arc_count = np.asarray(arc_count, np.int64).reshape(-1)
        B = self.num_utterances = len(node_count)
        self.num_frames = np.asarray(num_frames, np.int32).reshape(-1)
        self.reached_final = np.asarray(reached_final, bool).reshape(-1)
        self.cost = np.asarray(cost, np.float32).reshape(-1)
        self.acoustic_scale = np.asarray(acoustic_scale, np.float64).reshape(-1)
        if not (len(arc_count) == len(self.num_frames) == len(self.reached_final) == len(self.cost)
                == len(self.acoustic_scale) == B):
            raise ValueError("per-utterance arrays disagree in length")
        if (node_count < 0).any() or (arc_count < 0).any():
            raise ValueError("offsets must not decrease")
        self.node_off = np.r_[0, np.cumsum(node_count)].astype(np.int64)
        self.arc_off = np.r_[0, np.cumsum(arc_count)].astype(np.int64)
        N, A = self.num_nodes, self.num_arcs = int(self.node_off[-1]), int(self.arc_off[-1])
        if not (len(self.time) == len(self.state) == len(self.alpha) == len(self.beta) == N):
            raise ValueError("node arrays disagree with the node counts")
        if not (len(self.src) == len(self.dst) == len(self.arc) == len(self.lp) == A):
            raise ValueError("arc arrays disagree with the arc counts")
        if max(N, A) >= 2 ** 31 - 1:
            raise NotImplementedError("a batch holds fewer than 2^31 - 1 nodes and arcs")
        self.max_frames = int(self.num_frames.max()) if max_frames is None and B else int(max_frames or 0)
        self.num_classes = graph.max_ilabel if num_classes is None else int(num_classes)
        self.workspace_bytes = int(workspace_bytes)
        self.launches = 0                       # the kernel launches of the last operation that ran on the device
        self._host = None
        self._emission = {}                     # (T, C) -> the emission index of seq_objective
        self._build_levels()

    # ---- the level structure ------------------------------------------------------------
    def _build_levels(self):
        g, dev, B, N, A = self.graph, self.device, self.num_utterances, self.num_nodes, self.num_arcs
        i64 = dict(dtype=torch.int64, device=dev)
        self.node_off_d = torch.from_numpy(self.node_off).to(dev)
        self.arc_off_d = torch.from_numpy(self.arc_off).to(dev)
        counts = self.node_off_d[1:] - self.node_off_d[:-1]
        self.node_utt = torch.repeat_interleave(torch.arange(B, **i64), counts, output_size=N)
        self.arc_utt = torch.repeat_interleave(torch.arange(B, **i64), self.arc_off_d[1:] - self.arc_off_d[:-1],
                                               output_size=A)
        time, state = self.time.long(), self.state.long()
        src, dst = self.src.long(), self.dst.long()
        n_of = counts[self.arc_utt]
        bad = 0
        if N:
            bad = bad + ((state < 0) | (state >= g.num_states) | (time < 0)).sum()
        if A:
            bad = bad + ((src < 0) | (src >= n_of) | (dst < 0) | (dst >= n_of)).sum()
            bad = bad + ((self.arc < 0) | (self.arc >= len(g.src))).sum()
        if (N or A) and int(bad):               # one read-back for all the range checks
            raise ValueError("lattice arrays out of range: a node's state or time, an arc's end point "
                             "outside its utterance, or an arc index outside the graph")
        self.src_global = src + self.node_off_d[self.arc_utt]
        self.dst_global = dst + self.node_off_d[self.arc_utt]
        R = g.num_ranks + 1
        rank = g.device_arrays(dev)['rank'].long()
        t_max = int(time.max()) + 1 if N else 1
        key = time * R + rank[state] if N else time
        perm = _order((self.node_utt, key, state), (max(1, B), t_max * R, g.num_states)) if N else time
        ck = (self.node_utt * (t_max * R) + key)[perm]
        new = torch.ones(N, dtype=torch.bool, device=dev)
        if N > 1:
            new[1:] = ck[1:] != ck[:-1]
        level_sorted = torch.cumsum(new.long(), 0) - 1
        first = torch.nonzero(new).reshape(-1)
        L = self.num_levels = int(first.numel())
        node_level = torch.empty(N, **i64)
        node_level[perm] = level_sorted
        self.level_ptr = torch.cat([first, torch.full((1,), N, **i64)]).int()
        self.level_node = perm.int()
        self.node_level = node_level.int()
        level_utt = self.node_utt[perm][first]
        self.level_off_d = torch.searchsorted(level_utt, torch.arange(B + 1, **i64))
        self.level_off = self.level_off_d.cpu().numpy().astype(np.int64)
        if A:
            rises = node_level[self.src_global] < node_level[self.dst_global]
            ordered = self.src_global[1:] >= self.src_global[:-1] if A > 1 else rises
            if not bool(rises.all() & ordered.all()):
                raise ValueError("every lattice arc must lead to a higher (time, epsilon rank) level, and the "
                                 "arcs must be sorted by source node")
        ends = torch.arange(N + 1, **i64)
        order = torch.sort(self.dst_global, stable=True)[1] if A else self.dst_global
        self.in_arc = order.int()
        self.in_ptr = torch.searchsorted(self.dst_global[order].contiguous(), ends).int()
        self.out_ptr = torch.searchsorted(self.src_global.contiguous(), ends).int()
        self.frames_d = torch.from_numpy(self.num_frames).to(dev)
        self.reached_d = torch.from_numpy(self.reached_final.astype(np.int32)).to(dev)
        self.scale_d = torch.from_numpy(self.acoustic_scale).to(dev)

    @property
    def ilabel(self):
        """[A] the input label of every arc (0: epsilon), on the device.  The gather itself checks nothing, so an
        arc index changed behind the constructor's checks raises ValueError here: one reduction, one read-back"""
        if self.num_arcs and bool(((self.arc < 0) | (self.arc >= len(self.graph.src))).any()):
            raise ValueError("ilabel: an arc index outside the graph: the batch's index arrays are inconsistent")
        return self.graph.device_arrays(self.device)['il'][self.arc]

    # ---- construction ---------------------------------------------------------------------
    @classmethod
    def from_lattices(cls, lattices, device, graph=None, **kw):
        """Upload host `Lattice` objects over one graph (empty ones included: utterances without a
        lattice keep their place)."""
        lats = list(lattices)
        if graph is None:
            if not lats:
                raise ValueError("from_lattices needs a lattice or the graph")
            graph = lats[0].graph

        def cat(name, dtype):
            parts = [np.asarray(getattr(l, name), dtype) for l in lats]
            return torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, dtype))
        return cls(graph, device, cat('time', np.int32), cat('state', np.int32), cat('alpha', np.float32),
                   cat('beta', np.float32), cat('src', np.int32), cat('dst', np.int32), cat('arc', np.int64),
                   cat('lp', np.float32), [l.num_nodes for l in lats], [l.num_arcs for l in lats],
                   [l.num_frames for l in lats], [l.reached_final for l in lats], [l.cost for l in lats],
                   [l.acoustic_scale for l in lats], **kw)

    def lattices(self):
        """The batch as host `Lattice` objects, field for field what decode_lattice returns."""
        host = [getattr(self, k).cpu().numpy() for k in Lattice.FIELDS]
        out = []
        for b in range(self.num_utterances):
            ns = slice(self.node_off[b], self.node_off[b + 1])
            as_ = slice(self.arc_off[b], self.arc_off[b + 1])
            out.append(Lattice(self.graph, self.acoustic_scale[b], self.num_frames[b], self.cost[b],
                               self.reached_final[b], *[x[ns] for x in host[:4]], *[x[as_] for x in host[4:]]))
        return out

    def _host_batch(self):
        if self._host is None:
            self._host = LatticeBatch(self.lattices())
        return self._host

    def _native_path(self, name):
        """a batch on a GPU, unless ASR_LATTICE_<name>_NATIVE=0 (read per call)"""
        return self.device.type == 'cuda' and os.environ.get('ASR_LATTICE_%s_NATIVE' % name, '1') != '0'

    def _common_args(self):
        p = _native._p
        g = self.graph.device_arrays(self.device)
        head = (self.num_nodes, self.num_arcs, self.num_levels, _h(self.node_off), _h(self.arc_off),
                _h(self.level_off), p(self.node_off_d), p(self.arc_off_d), p(self.level_off_d), p(self.time),
                p(self.state), p(self.node_level), p(self.src), p(self.dst), p(self.arc), p(self.lp),
                p(self.level_ptr), p(self.level_node), p(self.in_ptr), p(self.in_arc), p(self.out_ptr),
                p(self.frames_d), p(self.reached_d), p(self.scale_d))
        tail = (self.graph.num_states, len(self.graph.src), p(g['w']), p(g['ol']), p(g['fin']), self.graph.start,
                int(THREADS_PER_WORKGROUP))
        return head, tail

    def _utterance_chunks(self, bytes_per_node, budget):
        """[b0, b1) ranges whose nodes fit the budget"""
        out, b0 = [], 0
        B = self.num_utterances
        while b0 < B:
            b1 = b0 + 1
            while b1 < B and (self.node_off[b1 + 1] - self.node_off[b0]) * bytes_per_node + 64 <= budget:
                b1 += 1
            if (self.node_off[b1] - self.node_off[b0]) * bytes_per_node + 64 > budget:
                raise ValueError("workspace_bytes = %d cannot hold utterance %d's %d nodes (%d bytes a node)"
                                 % (budget, b0, self.node_off[b1] - self.node_off[b0], bytes_per_node))
            out.append((b0, b1))
            b0 = b1
        return out

    @staticmethod
    def _check(code, what):
        if code == _native.ASR_EINVAL:
            raise ValueError("%s: %s" % (what, _native.lib().asr_strerror(code).decode()))
        _native.check(code, what)

    def _budget(self, workspace_bytes):
        return int(self.workspace_bytes if workspace_bytes is None else workspace_bytes)

    def _launch(self, entry, size, bytes_per_node, slack, workspace_bytes, lead, scales, args, supported=None):
        """The chunked launch of all six operations.  Asks asr_lattice_<op>_supported (nodes, arcs, levels and
        `size`, or `supported` in its place), plans the utterance chunks that fit workspace_bytes (default: the
        batch's) less `slack` at bytes_per_node, allocates one workspace for the biggest chunk
        (asr_lattice_<op>_workspace_bytes(nodes, *size)) and calls, once per chunk,
        entry(B, b0, b1 - b0, *lead, *head, *scales, *tail, *args, ws, nbytes, stream).  Returns the number of
        launches, for self.launches.  scales: (acoustic, LM) numbers, None for NaN (the lattice's own scale), or
        best_paths' two pointers.  What the launches wrote, the status words among it, is the caller's to read back."""
        L = _native.lib()
        stem = entry.rsplit('_', 1)[0]
        if not getattr(L, stem + '_supported')(self.num_nodes, self.num_arcs, self.num_levels,
                                                *(size if supported is None else supported)):
            raise NotImplementedError("%s: the batch is too large" % entry)
        chunks = self._utterance_chunks(bytes_per_node, self._budget(workspace_bytes) - slack)
        nbytes = getattr(L, stem + '_workspace_bytes')(
            max(int(self.node_off[b1] - self.node_off[b0]) for b0, b1 in chunks), *size)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        head, tail = self._common_args()
        scales = [x if isinstance(x, ctypes.c_void_p) else float('nan' if x is None else x) for x in scales]
        run, B = getattr(L, entry), self.num_utterances
        for b0, b1 in chunks:
            self._check(run(B, b0, b1 - b0, *lead, *head, *scales, *tail, *args, _native._p(ws), nbytes,
                            _native._stream()), entry)
        return len(chunks)

    @staticmethod
    def _refuse_bad_status(status, entry, mask=-1):
        """status: the launches' status words on the host; mask: the bits that say the index arrays were refused"""
        if (status & mask).any():
            raise ValueError("%s: the batch's index arrays are inconsistent" % entry)

    def _redo_on_host(self, out, redo, warning, run):
        """out with the utterances `redo` replaced by run(LatticeBatch of them), the host twin's results"""
        if redo:
            warnings.warn(warning)
            lats = self._host_batch().lattices
            for b, r in zip(redo, run(LatticeBatch([lats[b] for b in redo]))):
                out[b] = r
        return out

    # ---- the tropical sweep -----------------------------------------------------------------
    def best_paths(self, acoustic_scales=None, lm_scales=1.0, workspace_bytes=None):
        """The best path of every lattice under every (acoustic scale, LM scale) pair.

        acoustic_scales: a float, None (each lattice's own search scale) or a sequence of those;
        lm_scales: a float or a sequence of the same length.  Returns one list per pair (a single
        float or None is one pair), each what LatticeBatch(lattices).best_paths(sc, lm) returns:
        (words, cost, graph_cost, acoustic_cost) per utterance, bit for bit.  On a GPU all pairs
        and utterances are one launch of asr_lattice_bestpath_f64, or several when workspace_bytes
        (default: the batch's) does not hold 12 bytes per node and pair at once."""
        acs, _ = _scale_list(acoustic_scales)
        lms, one = _scale_list(lm_scales)
        if one:
            lms = lms * len(acs)
        if len(lms) != len(acs):
            raise ValueError("lm_scales must be a float or as long as acoustic_scales")
        P, B = len(acs), self.num_utterances
        if not self._native_path('DP'):
            hb = self._host_batch()
            with np.errstate(invalid='ignore'):
                return [hb.best_paths(sc, lm) for sc, lm in zip(acs, lms)]
        none = ([], INF, INF, INF)
        if P == 0 or B == 0 or self.num_nodes == 0:
            return [[none] * B for _ in range(P)]
        dev, p = self.device, _native._p
        per_launch = max(1, min(P, (self._budget(workspace_bytes) - 64) // max(1, 12 * self.num_nodes)))
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        ac_d = torch.tensor([float('nan') if a is None else float(a) for a in acs], **f64)
        lm_d = torch.tensor([float(x) for x in lms], **f64)
        cost = torch.empty((P, B, 3), **f64)
        n_words = torch.zeros((P, B), **i32)
        words = torch.zeros((P, max(1, self.num_levels)), **i32)
        status = torch.zeros((P, B), **i32)
        self.launches = sum(                    # a group of pairs: the same chunks and workspace size every time
            self._launch('asr_lattice_bestpath_f64', (per_launch,), 12 * per_launch, 0, workspace_bytes,
                         (min(per_launch, P - p0),), (p(ac_d[p0:]), p(lm_d[p0:])),
                         (p(cost[p0:]), p(n_words[p0:]), p(words[p0:]), p(status[p0:])), supported=())
            for p0 in range(0, P, per_launch))
        cost_h, nw_h, words_h = cost.cpu().numpy(), n_words.cpu().numpy(), words.cpu().numpy()
        self._refuse_bad_status(status.cpu().numpy(), 'asr_lattice_bestpath_f64')
        out = []
        for k in range(P):
            row = []
            for b in range(B):
                c = cost_h[k, b]
                if not c[0] < INF:
                    row.append(none)
                    continue
                o = int(self.level_off[b])
                row.append((words_h[k, o:o + nw_h[k, b]].tolist(), float(c[0]), float(c[1]), float(c[2])))
            out.append(row)
        return out

    # ---- n-best lists --------------------------------------------------------------------------
    def nbest(self, n, acoustic_scale=None, lm_scale=1.0, workspace_bytes=None):
        """The n cheapest DISTINCT word sequences of every lattice: one [(words, cost)] per utterance,
        sorted by (cost, words); the semantics are LatticeBatch.nbest's (a
        k-best dynamic programme over the levels, sequences told apart by a 64-bit hash of their
        words, ties at the n-th cost cut by (length, hash) where Lattice.nbest cuts by the words).

        On a GPU all utterances are one launch of asr_lattice_nbest_f64, or several when
        workspace_bytes (default: the batch's) does not hold 28 n + 4 bytes per node at once.  A
        batch of CPU tensors, ASR_LATTICE_NBEST_NATIVE=0 (read per call) and n above
        NBEST_DEVICE_MAX run LatticeBatch.nbest on a copy: the same bits in every case."""
        n = int(n)
        B = self.num_utterances
        if not (self._native_path('NBEST') and n <= NBEST_DEVICE_MAX):
            return self._host_batch().nbest(n, acoustic_scale, lm_scale)
        if n < 1 or B == 0 or self.num_nodes == 0:
            return [[] for _ in range(B)]
        count, status, cost, n_words, words = self._nbest_launch(n, acoustic_scale, lm_scale, workspace_bytes)
        packed = torch.cat([count, status, n_words.reshape(-1)]).cpu().numpy()     # the small ones in one read-back
        count_h, status_h, nw_h = packed[:B], packed[B:2 * B], packed[2 * B:].reshape(B, n)
        self._refuse_bad_status(status_h, 'asr_lattice_nbest_f64')
        cost_h, words_h = cost.cpu().numpy(), words.cpu().numpy()
        levels = np.diff(self.level_off)
        utt, rows, costs = [], [], []
        for b in np.nonzero(count_h)[0].tolist():
            base, lv = n * int(self.level_off[b]), int(levels[b])
            for i in range(int(count_h[b])):
                o = base + i * lv
                utt.append(b)
                rows.append(words_h[o:o + nw_h[b, i]].tolist())
                costs.append(float(cost_h[b, i]))
        return nbest_lists(B, utt, rows, costs)

    def _nbest_launch(self, n, acoustic_scale, lm_scale, workspace_bytes):
        """the launches of nbest alone: (count [B], status [B], cost [B, n], n_words [B, n], words [n L]) on
        the device, as asr_lattice_nbest_f64 leaves them"""
        B, dev, p = self.num_utterances, self.device, _native._p
        i32 = dict(dtype=torch.int32, device=dev)
        count, status = torch.zeros(B, **i32), torch.zeros(B, **i32)
        cost = torch.empty((B, n), dtype=torch.float64, device=dev)
        n_words = torch.zeros((B, n), **i32)
        words = torch.zeros(n * max(1, self.num_levels), **i32)
        self.launches = self._launch(           # 128: the rounding of the six arrays
            'asr_lattice_nbest_f64', (n,), 28 * n + 4, 128, workspace_bytes, (n,), (acoustic_scale, lm_scale),
            (p(count), p(cost), p(n_words), p(words), p(status)))
        return count, status, cost, n_words, words

    def sentences(self, n, **kw):
        """the word lists of nbest(n) per utterance: what AttentionDecoderTCN.score_sentences takes"""
        return [[w for w, _ in row] for row in self.nbest(n, **kw)]

    # ---- minimum-Bayes-risk decoding -------------------------------------------------------------
    def mbr(self, acoustic_scale=None, lm_scale=1.0, max_iterations=16, hypotheses=None, workspace_bytes=None,
            arc_cond=None, end_cond=None, max_words=None):
        """Minimum-Bayes-risk decoding of every lattice: one MBRResult per utterance (words, confidence,
        frames, risk, iterations, sausage); the semantics are LatticeBatch.mbr's (DESIGN.md section
        4.23, include/asr_amd.h): the word sequence of the least expected word edit distance under the
        lattice's path distribution at these scales, from `hypotheses` (a word list per utterance) or
        the best path, by at most max(1, max_iterations) edit-distance forward-backward passes.

        On a GPU all utterances and all iterations are one launch of asr_lattice_mbr_f64, or several
        when workspace_bytes (default: the batch's) does not hold 16 (2 max_words + 2) + 8 bytes per
        node at once; self.launches counts them.  max_words (default: the most levels of an utterance,
        at most MBR_DEVICE_MAX_WORDS) is the longest hypothesis the launch has columns for.
        arc_cond / end_cond (fp64, per arc / node, numpy or tensors): LatticeBatch.conditionals'
        values instead of the kernel's own forward pass; with them the result equals the twin's with ==.
        A batch of CPU tensors and ASR_LATTICE_MBR_NATIVE=0 (read per call) run LatticeBatch.mbr on a
        copy; so do, with one warning per call, the utterances whose hypothesis outgrew max_words or
        whose sausage outgrew its buffer."""
        B = self.num_utterances
        if hypotheses is not None:
            if len(hypotheses) != B:
                raise ValueError("hypotheses must hold one word list per utterance")
            hypotheses = [[int(w) for w in h] for h in hypotheses]
            if any(w <= 0 for h in hypotheses for w in h):
                raise ValueError("hypotheses hold word labels > 0")

        def host(x):
            return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
        self.launches = 0
        if not self._native_path('MBR'):
            return self._host_batch().mbr(acoustic_scale, lm_scale, max_iterations, hypotheses, host(arc_cond),
                                          host(end_cond))
        if B == 0 or self.num_nodes == 0:
            return [MBR_NONE] * B
        levels = np.diff(self.level_off)
        W = int(levels.max()) if max_words is None else int(max_words)
        W = max(1, min(W, MBR_DEVICE_MAX_WORDS))
        if getattr(self, '_mbr_labels', None) is None:     # the graph's distinct words, and 0: no slot holds more
            ol = np.asarray(self.graph.olabel)
            self._mbr_labels = int(len(np.unique(ol[ol != 0]))) + 1
        cap = int(MBR_SAUSAGE_ENTRIES) or min(self._mbr_labels, 64) * (2 * W + 2)
        dev, p = self.device, _native._p
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)

        def cond(x, n, what):
            if x is None:
                return None
            x = torch.as_tensor(x).to(dev, torch.float64).contiguous()
            if x.numel() != n:
                raise ValueError("%s must have %d entries" % (what, n))
            return x
        arc_cond, end_cond = cond(arc_cond, self.num_arcs, 'arc_cond'), cond(end_cond, self.num_nodes, 'end_cond')
        init_w = init_n = None
        if hypotheses is not None:
            rows = np.zeros((B, W), np.int32)
            counts = np.zeros(B, np.int32)
            for b, h in enumerate(hypotheses):
                counts[b] = len(h) if len(h) <= W else -1      # -1: the kernel hands the utterance back
                if len(h) <= W:
                    rows[b, :len(h)] = h
            init_w, init_n = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
        small = torch.zeros((4, B), **i32)              # words, iterations, status, sausage entries
        words, frames = torch.zeros((B, W), **i32), torch.zeros((B, W), **i32)
        conf, risk = torch.zeros((B, W), **f64), torch.full((B,), INF, **f64)
        table = torch.full((3, B, cap), -1, dtype=torch.int64, device=dev)
        self.launches = self._launch(
            'asr_lattice_mbr_f64', (W,), 16 * (2 * W + 2) + 8, 64, workspace_bytes, (), (acoustic_scale, lm_scale),
            (p(arc_cond), p(end_cond), p(init_w), p(init_n), int(max_iterations), W, cap, p(small[0]), p(words),
             p(conf), p(frames), p(risk), p(small[1]), p(small[2]), p(small[3]), p(table[0]), p(table[1]),
             p(table[2])))
        nw_h, it_h, status_h, _ = small.cpu().numpy()
        self._refuse_bad_status(status_h, 'asr_lattice_mbr_f64', 1)
        used = torch.nonzero(((table[0] >= 0) & (table[1] > 0)).reshape(-1)).reshape(-1)    # the entries alone cross
        t_utt = torch.div(used, cap, rounding_mode='floor').cpu().numpy()
        t_key, t_gamma, t_tau = (table[j].reshape(-1)[used].cpu().numpy() for j in range(3))
        tables = [{} for _ in range(B)]
        for b, k, g, t in zip(t_utt.tolist(), t_key.tolist(), t_gamma.tolist(), t_tau.tolist()):
            tables[b][(k >> 32, k & 0xFFFFFFFF)] = (g, t)
        words_h, frames_h, conf_h, risk_h = words.cpu().numpy(), frames.cpu().numpy(), conf.cpu().numpy(), \
            risk.cpu().numpy()
        out = []
        for b in range(B):
            if status_h[b] or not risk_h[b] < INF:
                out.append(MBR_NONE)
                continue
            n = int(nw_h[b])
            out.append(MBRResult(words_h[b, :n].tolist(), conf_h[b, :n].tolist(), frames_h[b, :n].tolist(),
                                 float(risk_h[b]), int(it_h[b]), mbr_sausage(tables[b])))
        redo = np.nonzero(status_h)[0].tolist()

        def twin(sub):
            ac, ec = host(arc_cond), host(end_cond)
            pick = np.concatenate
            return sub.mbr(acoustic_scale, lm_scale, max_iterations,
                           None if hypotheses is None else [hypotheses[b] for b in redo],
                           None if ac is None else pick([ac[self.arc_off[b]:self.arc_off[b + 1]] for b in redo]),
                           None if ec is None else pick([ec[self.node_off[b]:self.node_off[b + 1]] for b in redo]))
        return self._redo_on_host(out, redo, "mbr: %d of %d utterances outgrew the device's %d words a hypothesis or "
                                  "%d sausage entries and were redone on the host" % (len(redo), B, W, cap), twin)

    def expected_errors(self, sentences, acoustic_scale=None, lm_scale=1.0, **kw):
        """The expected word edit distance of given sentences over their lattices: `sentences` holds a
        list of word lists per utterance (the shape sentences(n) returns); returns the risks in that
        shape (+inf: no lattice).  mbr(max_iterations=0, hypotheses=...) once per list position, so n
        sentences an utterance are n launches (self.launches counts them all), each with its own
        forward pass, table and read-back: the hand-over that lets a rescoring stage weigh a candidate by its expected word error."""
        if len(sentences) != self.num_utterances:
            raise ValueError("sentences must hold one list per utterance")
        out = [[] for _ in sentences]
        launches = 0
        for i in range(max([len(s) for s in sentences] + [0])):
            res = self.mbr(acoustic_scale, lm_scale, 0, [s[i] if i < len(s) else [] for s in sentences], **kw)
            launches += self.launches
            for b, s in enumerate(sentences):
                if i < len(s):
                    out[b].append(res[b].risk)
        self.launches = launches
        return out

    # ---- the lattice oracle ------------------------------------------------------------------------
    def oracle(self, references, acoustic_scale=None, lm_scale=1.0, workspace_bytes=None):
        """The lattice oracle (Kaldi's lattice-oracle): per utterance the complete path whose words are nearest
        to the reference (a list of labels > 0 per utterance) in word edit distance, one OracleResult each
        (errors, substitutions, insertions, deletions, correct, words, ref_frames, cost; ORACLE_NONE where the
        lattice has no complete path); the semantics are LatticeBatch.oracle's (DESIGN.md section 4.25,
        include/asr_amd.h), and so are the results, with ==.  oracle_error_rate sums them up.

        On a GPU all utterances are one launch of asr_lattice_oracle_i32, or several when workspace_bytes
        (default: the batch's) does not hold 4 (max_words + 1) bytes per node at once, max_words being the
        longest reference of the call; self.launches counts them.  A batch of CPU tensors and
        ASR_LATTICE_ORACLE_NATIVE=0 (read per call) run LatticeBatch.oracle on a copy; so do, with one warning
        per call, the utterances whose reference is longer than ORACLE_DEVICE_MAX_WORDS."""
        B = self.num_utterances
        refs = _oracle_references(references, B)
        self.launches = 0
        if not self._native_path('ORACLE'):
            return self._host_batch().oracle(refs, acoustic_scale, lm_scale)
        if B == 0 or self.num_nodes == 0:
            return [ORACLE_NONE] * B
        limit = max(1, min(int(ORACLE_DEVICE_MAX_WORDS), 1023))
        redo = [b for b, r in enumerate(refs) if len(r) > limit]
        W = max([1] + [len(r) for r in refs if len(r) <= limit])
        dev, p = self.device, _native._p
        rows = np.zeros((B, W), np.int32)
        counts = np.zeros(B, np.int32)
        for b, r in enumerate(refs):
            if len(r) <= limit:                 # the others: an empty reference here, redone on the host below
                rows[b, :len(r)] = r
                counts[b] = len(r)
        ref_w, ref_n = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        small = torch.zeros((7, B), **i32)              # errors, status, words, then sub, ins, del, cor as [B, 4]
        counts_d = small[3:].reshape(B, 4)
        words = torch.zeros(max(1, self.num_levels), **i32)
        frames = torch.zeros((B, W), **i32)
        cost = torch.full((B,), INF, dtype=torch.float64, device=dev)
        self.launches = self._launch(
            'asr_lattice_oracle_i32', (W,), 4 * (W + 1), 64, workspace_bytes, (), (acoustic_scale, lm_scale),
            (p(ref_w), p(ref_n), W, p(small[0]), p(counts_d), p(small[2]), p(words), p(frames), p(cost), p(small[1])))
        small_h = small.cpu().numpy()
        err_h, status_h, nw_h, ops_h = small_h[0], small_h[1], small_h[2], small_h[3:].reshape(B, 4)
        self._refuse_bad_status(status_h, 'asr_lattice_oracle_i32', 1)
        words_h, frames_h, cost_h = words.cpu().numpy(), frames.cpu().numpy(), cost.cpu().numpy()
        out = []
        for b in range(B):
            if err_h[b] < 0:
                out.append(ORACLE_NONE)
                continue
            o = int(self.level_off[b])
            n_sub, n_ins, n_del, n_cor = (int(x) for x in ops_h[b])
            out.append(OracleResult(int(err_h[b]), n_sub, n_ins, n_del, n_cor, words_h[o:o + nw_h[b]].tolist(),
                                    frames_h[b, :len(refs[b])].tolist(), float(cost_h[b])))
        return self._redo_on_host(out, redo, "oracle: %d of %d utterances have a reference of more than the device's "
                                  "%d words and were redone on the host" % (len(redo), B, limit),
                                  lambda sub: sub.oracle([refs[b] for b in redo], acoustic_scale, lm_scale))

    def depth(self):
        """per utterance the emitting lattice arcs per frame (Kaldi's lattice-depth), 0.0 for an empty lattice:
        LatticeBatch.depth's numbers, counted with torch ops on the batch's device"""
        B = self.num_utterances
        if B == 0:
            return []
        arcs = torch.zeros(B, dtype=torch.int64, device=self.device)
        if self.num_arcs:
            arcs.index_add_(0, self.arc_utt, (self.ilabel != 0).long())
        arcs = arcs.cpu().numpy()
        nodes = np.diff(self.node_off)
        return [float(int(arcs[b])) / float(self.num_frames[b]) if nodes[b] and self.num_frames[b] >= 1 else 0.0
                for b in range(B)]

    # ---- rescoring with a back-off n-gram LM --------------------------------------------------
    def rescore_lm(self, lm, label_map=None, scale=1.0, lattice_beam=None, oov_cost=INF, max_lm_states=None,
                   workspace_bytes=None):
        """lattice o LM (Kaldi's lattice-lmrescore under the back-off reading): another DeviceLatticeBatch
        on this device over a RescoredGraph of its own, with alpha, beta and cost recomputed, so best_paths,
        nbest, sentences, posteriors and mbr run on it unchanged.  att_speech.lattice_lm states the semantics
        (DESIGN.md section 4.24).

        lm: a BackoffLm, an LmFst or a file name; label_map: output label of the graph -> label of the LM
        (None: matched by name when both have symbol tables, else the identity; lattice_lm.lm_label_map for
        graphs of DecodingGraph.from_graph_generator); scale multiplies the LM costs (-1 takes a first-pass
        LM out, approximately: the first pass treated back-off arcs as ordinary epsilons); lattice_beam
        prunes against the new best (None: everything on a complete finite path); oov_cost: the cost of an
        arc whose word the LM does not know (inf drops it).

        On a GPU: asr_lattice_lmrescore_expand / _emit per launch (several launches when workspace_bytes,
        default the batch's, does not hold 4 max_lm_states bytes per node at once) and one
        asr_lattice_lmrescore_sweep; self.launches counts them.  An utterance with more than max_lm_states
        (default 256, at most 1024) LM states on one node is redone by the numpy twin, with one warning per
        call.  A batch of CPU tensors and ASR_LATTICE_RESCORE_NATIVE=0 (read per call) run the twin: the
        same bits.  result.stats: max_lm_states, nodes_in, nodes_out, arcs_in, arcs_out, dropped_arcs,
        redone_on_host."""
        from att_speech.lattice_lm import rescore_device_batch
        return rescore_device_batch(self, lm, label_map, scale, lattice_beam, oov_cost, max_lm_states,
                                    workspace_bytes)

    # ---- the log-semiring pass ----------------------------------------------------------------
    def posteriors(self, acoustic_scale=None, lm_scale=1.0, workspace_bytes=None):
        """Arc and node posteriors under the path weights exp(-(sum of x + lm_scale * end)), x and end
        as in best_paths: a LatticePosteriors (log_z [B], arc_log_post [A], node_log_post [N] in
        fp64, frame_posteriors(), word_posteriors()).  On a GPU one launch of
        asr_lattice_posterior_f64 does forward and backward (several when workspace_bytes does not
        hold 16 bytes per node at once; self.launches counts them); two runs give the same bits."""
        if not self._native_path('DP'):
            post = self._host_batch().posteriors(acoustic_scale, lm_scale)
            if self.device.type == 'cuda':
                post = LatticePosteriors(self, *[torch.from_numpy(np.asarray(x, np.float64)).to(self.device) for x in
                                                 (post.log_z, post.arc_log_post, post.node_log_post)],
                                         acoustic_scale, lm_scale)
            return post
        B, dev, p = self.num_utterances, self.device, _native._p
        f64 = dict(dtype=torch.float64, device=dev)
        log_z = torch.full((B,), -INF, **f64)
        arc_post = torch.full((self.num_arcs,), -INF, **f64)
        node_post = torch.full((self.num_nodes,), -INF, **f64)
        res = LatticePosteriors(self, log_z, arc_post, node_post, acoustic_scale, lm_scale)
        if B == 0 or self.num_nodes == 0:
            return res
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.launches = self._launch('asr_lattice_posterior_f64', (), 16, 0, workspace_bytes, (),
                                     (acoustic_scale, lm_scale), (p(log_z), p(arc_post), p(node_post), p(status)))
        self._refuse_bad_status(status.cpu().numpy(), 'asr_lattice_posterior_f64')
        return res

    # ---- sequence-discriminative training statistics ------------------------------------------
    def _emission_index(self, T, C):
        """The emitting arcs grouped by their entry of a [T, B, C] tensor, built once per batch and shape
        with torch ops on the device: em_arc [E] int32 the emitting arcs by (utterance, frame, class, arc),
        em_ptr [S+1] int32 the segments of equal (utterance, frame, class), em_key [S] int64 their offsets
        ((k-1) B + b) C + class, em_off [B+1] int64 the segments of every utterance.  Raises ValueError when
        an arc reads a class or a frame beyond [T, B, C]."""
        hit = self._emission.get((T, C))
        if hit is not None:
            return hit
        dev, B, A = self.device, self.num_utterances, self.num_arcs
        i64 = dict(dtype=torch.int64, device=dev)
        if A:
            il = self.ilabel.long()
            k = self.time.long()[self.dst_global]
            arcs = torch.nonzero(il > 0).reshape(-1)
            il, k, utt = il[arcs], k[arcs], self.arc_utt[arcs]
            if int(arcs.numel()) and bool(((il > C) | (k > T) | (k < 1)).any()):
                raise ValueError("seq_objective: the lattice has classes or frames beyond [T, B, C] = %s"
                                 % ((T, B, C),))
        else:
            arcs = il = k = utt = torch.zeros(0, **i64)
        E = int(arcs.numel())
        flat = ((k - 1) * B + utt) * C + (il - 1)
        order = torch.sort(utt * (T * B * C) + flat, stable=True)[1] if E else arcs    # arcs ascend already
        flat, utt = flat[order], utt[order]
        new = torch.ones(E, dtype=torch.bool, device=dev)
        if E > 1:
            new[1:] = (flat[1:] != flat[:-1]) | (utt[1:] != utt[:-1])
        first = torch.nonzero(new).reshape(-1)
        hit = dict(E=E, S=int(first.numel()), em_arc=arcs[order].int().contiguous(),
                   em_ptr=torch.cat([first, torch.full((1,), E, **i64)]).int(),
                   em_key=flat[first].contiguous(),
                   em_off=torch.searchsorted(utt[first].contiguous(), torch.arange(B + 1, **i64)))
        self._emission[(T, C)] = hit
        return hit

    def seq_objective(self, log_probs, ref=None, criterion='mmi', acoustic_scale=None, lm_scale=1.0, boost=0.0,
                      workspace_bytes=None):
        """The lattice MMI / boosted MMI denominator ('mmi': log Z and the arc posteriors) or the sMBR
        objective ('smbr': the expected frame accuracy against `ref` and its derivative) of every lattice,
        with the arc scores read from the LIVE log_probs [T, B, C] float32 instead of the lp stored at decode
        time, so lattices made by a stale model can be reused.  LatticeBatch.seq_objective states the
        semantics.  ref: [B, T] int32 classes per frame (CTCAlignment.frames, -1
        padding) or None; boost >= 0 adds boost per correct frame to a path's cost (boosted MMI).

        Returns (objective [B] f64, arc_grad [A] f64, occ [T, B, C] float32) on the batch's device;
        d objective[b] / d log_probs[t, b, c] = acoustic_scale occ[t, b, c].  On a GPU one launch of
        asr_lattice_seqtrain_f64 does the sweeps, the arcs and the scatter into occ (several launches when
        workspace_bytes, default the batch's, does not hold 32 bytes per node at once; self.launches counts
        them); two runs give the same bits.  A batch of CPU tensors and ASR_LATTICE_TRAIN_NATIVE=0 (read per
        call) run the twin."""
        if criterion not in ('mmi', 'smbr'):
            raise ValueError("criterion must be 'mmi' or 'smbr', not %r" % (criterion,))
        if not float(boost) >= 0.0 or float(boost) == INF:
            raise ValueError("boost must be finite and >= 0")
        B, dev, p = self.num_utterances, self.device, _native._p
        if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3 or log_probs.size(1) != B:
            raise ValueError("log_probs must be a [T, B = %d, C] tensor" % B)
        if log_probs.device != dev:
            raise ValueError("log_probs is on %s, the batch on %s" % (log_probs.device, dev))
        T, _, C = log_probs.shape
        if ref is not None:
            ref = torch.as_tensor(ref)
            if tuple(ref.shape) != (B, T) or ref.dtype.is_floating_point:
                raise ValueError("ref must be an integer [B, T] = %s tensor, not %s" % ((B, T), tuple(ref.shape)))
        if not self._native_path('TRAIN'):
            out = self._host_batch().seq_objective(log_probs, ref, criterion, acoustic_scale, lm_scale, boost)
            return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in out)
        if log_probs.dtype != torch.float32:
            raise ValueError("log_probs must be float32 on the device")
        smbr = criterion == 'smbr'
        f64 = dict(dtype=torch.float64, device=dev)
        objective = torch.full((B,), 0.0 if smbr else -INF, **f64)
        arc_grad = torch.zeros(self.num_arcs, **f64)
        occ = torch.zeros((T, B, C), dtype=torch.float32, device=dev)
        self.launches = 0
        if B == 0 or self.num_nodes == 0:
            return objective, arc_grad, occ
        em = self._emission_index(int(T), int(C))
        lp = log_probs.detach().contiguous()
        ref_d = None if ref is None else ref.to(dev, torch.int32).contiguous()
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        il = self.graph.device_arrays(dev)['il']
        self.launches = self._launch(
            'asr_lattice_seqtrain_f64', (), 32, 0, workspace_bytes, (), (acoustic_scale, lm_scale),
            (p(il), p(lp), int(T), int(C), p(ref_d), 1 if smbr else 0, float(boost), em['E'], em['S'],
             p(em['em_arc']), p(em['em_ptr']), p(em['em_key']), p(em['em_off']), p(objective), p(arc_grad), p(occ),
             p(status)))
        if status.cpu().numpy().any():
            raise ValueError("asr_lattice_seqtrain_f64: the batch's index arrays are inconsistent, or an arc "
                             "reads a frame or class beyond [T, B, C]")
        return objective, arc_grad, occ


def decode_lattice_device(log_probs, lens, graph, beam=16.0, lattice_beam=8.0, acoustic_scale=1.0,
                          allow_partial=True, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """decode_lattice whose lattices stay where the search left them: (DeviceLatticeBatch,
    redone_on_host).  The same launch and the same canonical sort on the device; nothing but the
    per-utterance counts crosses to the host.  batch.lattices() is decode_lattice's list.  An
    utterance that outgrows the device workspace is decoded by decode_lattice_host as there (one
    warning per call) and its lattice is uploaded into its place.  CPU tensors, or
    ASR_WFST_LATTICE_NATIVE=0: the host search, uploaded to the tensor's device."""
    lp, lens_np = _validate(log_probs, lens, graph, beam, lattice_beam)
    T, B, C = lp.shape
    kw = dict(graph=graph, max_frames=T, num_classes=C, workspace_bytes=workspace_bytes)
    native = lp.is_cuda and os.environ.get('ASR_WFST_LATTICE_NATIVE', '1') != '0'
    if not native or B == 0 or T == 0:
        lats, _ = decode_lattice_host(lp.cpu().numpy(), lens_np, graph, beam, lattice_beam, acoustic_scale,
                                      allow_partial)
        return DeviceLatticeBatch.from_lattices(lats, lp.device, **kw), []
    lp = lp.contiguous()
    cost, final, n_nodes, n_arcs, overflow, packed = _decode_device(
        lp, lens_np, graph, beam, lattice_beam, acoustic_scale, allow_partial, int(workspace_bytes), to_host=False)
    cost, final, n_nodes, n_arcs, overflow = (x.cpu().numpy() for x in (cost, final, n_nodes, n_arcs, overflow))
    redo = np.nonzero(overflow)[0].tolist()
    n_nodes = np.where(overflow != 0, 0, n_nodes).astype(np.int64)
    n_arcs = np.where(overflow != 0, 0, n_arcs).astype(np.int64)
    gone = n_nodes == 0
    cost = np.where(gone, np.float32(INF), cost)
    reached = np.where(gone, False, final != 0)
    n_arcs = np.where(gone, 0, n_arcs)
    if redo:
        warnings.warn("decode_lattice: %d of %d utterances outgrew the device workspace (%s; "
                      "workspace_bytes = %d) and were decoded on the host"
                      % (len(redo), B, ', '.join(sorted({OVERFLOW_NAMES.get(int(overflow[b]), '?') for b in redo})),
                         workspace_bytes))
        idx = torch.as_tensor(redo, device=lp.device)
        h, _ = decode_lattice_host(lp[:, idx].cpu().numpy(), lens_np[redo], graph, beam, lattice_beam,
                                   acoustic_scale, allow_partial)
        pieces = [list(torch.split(x, (n_nodes if j < 4 else n_arcs).tolist())) for j, x in enumerate(packed)]
        for lat, b in zip(h, redo):
            for j, name in enumerate(Lattice.FIELDS):
                pieces[j][b] = torch.from_numpy(np.asarray(getattr(lat, name))).to(lp.device).to(packed[j].dtype)
            n_nodes[b], n_arcs[b] = lat.num_nodes, lat.num_arcs
            cost[b], reached[b] = lat.cost, lat.reached_final
        packed = [torch.cat(x) for x in pieces]
    kw.pop('graph')
    batch = DeviceLatticeBatch(graph, lp.device, *packed, n_nodes, n_arcs, lens_np, reached, cost,
                               np.full(B, float(acoustic_scale)), **kw)
    return batch, redo
