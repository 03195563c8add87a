"""att_speech.modules.beam_search — the searches of the reference
(att_speech/modules/beam_search.py): plain BeamSearch (:13-182), the search
reachable without an external LM FST (`AttentionDecoderTCN.decode`,
tcn.py:527-531), and the LM-fused BeamSearchLM (:185-363), RescoreSearchLM
(:366-403) and GraphSearch (:406-648) for an `att_speech.lm_fst.LmFst`.

Same step semantics and the same quirks, with the hypothesis re-indexing done
by device-side gathers instead of the reference's Python `batch x beam` double
loop (:108-124) and ONE host read-back per step for the finished-hypothesis
bookkeeping instead of `.item()` calls inside loops (:58-81).

DeviceBeamSearch, DeviceBeamSearchLM and DeviceGraphSearch keep all of their state on the device
(include/asr_amd.h: asr_beam_step_f32; the launches of csrc/beam_lm.hip).  `graph_sentences`,
`sentence_trie` and DeviceForcedScorer (asr_forced_level_f32, csrc/forced_score.hip) serve
`AttentionDecoderTCN.score_sentences`, the forced rescoring of a lattice's sentences.

Quirks kept on purpose (bit-compatible results):
  * `is_eos_best` is computed per hypothesis ([B*beam]) but indexed with the
    batch id (:73) — i.e. it looks at hypothesis `batch_id`, not at the batch's
    best beam;
  * `best_finished_scores_elements['acoustic']` aliases `best_finished_scores`
    (:30-32), so the raw EOS score overwrites the length-normalised one (:77-78).
"""
import numpy as np
import torch

from att_speech import fst_utils


class BeamSearch(object):
    def __init__(self, batch_size, beam_size, device, num_classes,
                 length_normalization, keep_eos_score=False):
        self.scores = torch.zeros(batch_size * beam_size, device=device)
        self.estimations = None
        self.finished_count = [0 for _ in range(batch_size)]
        self.best_finished = [[] for _ in range(batch_size)]
        self.best_finished_scores = [float('-inf')] * batch_size
        self.best_finished_scores_elements = {'acoustic': self.best_finished_scores}
        self.beam_size = beam_size
        self.batch_size = batch_size
        self.num_classes = num_classes
        self.length_normalization = length_normalization
        self.min_eos = None
        self.keep_eos_score = keep_eos_score
        self.coverage = None
        self.attentions = None
        self.print_debug = False
        self.gather_attentions = False

    def _save_best_finished(self, global_scores):
        """(:58-81) for each utterance: extended beam with the best EOS score."""
        B, beam = self.batch_size, self.beam_size
        scores = global_scores[:, -1].contiguous().view(B, -1)
        eos_scores = scores / (self.estimations.size(1) ** self.length_normalization)
        is_eos_best = torch.argmax(global_scores, dim=1) == global_scores.size(1) - 1
        ind = torch.argmax(eos_scores, dim=1)
        best_norm = eos_scores.gather(1, ind[:, None]).squeeze(1)
        best_raw = scores.gather(1, ind[:, None]).squeeze(1)
        host = torch.stack([is_eos_best[:B].to(best_norm.dtype), ind.to(best_norm.dtype),
                            best_norm, best_raw]).cpu()         # one read-back per step
        for b in range(B):
            if host[0, b] != 0 and self.finished_count[b] <= beam:
                self.finished_count[b] += 1
                if self.best_finished_scores[b] < float(host[2, b]):
                    # aliased lists: the raw score is what stays (:76-78)
                    self.best_finished_scores[b] = float(host[3, b])
                    self.best_finished[b] = self.estimations[b * beam + int(host[1, b])]

    def _get_topk(self, scores):
        """(:83-98)"""
        if self.beam_size < scores.size(1):
            return torch.topk(scores, self.beam_size, dim=1)
        new_scores, best_it = torch.topk(scores, scores.size(1), dim=1)
        to_repeat = self.beam_size - scores.size(1)
        no_scores = (torch.ones_like(new_scores[:, -1:]) * float('-inf')).repeat(1, to_repeat)
        new_scores = torch.cat((new_scores, no_scores), dim=1)
        best_it = torch.cat((best_it, best_it[:, -1:].repeat(1, to_repeat)), dim=1)
        return new_scores, best_it

    def step(self, logits, *args, **kwargs):
        """(:147-175) logits [1, B*beam, C] -> (new input ids [B*beam],
        state mapping [B*beam])."""
        local_scores = torch.nn.functional.log_softmax(logits.squeeze(0), dim=1)
        global_scores = local_scores + self.scores.unsqueeze(1).repeat(1, self.num_classes)
        if self.estimations is not None:
            self._save_best_finished(global_scores)
        new_scores, best_it = self._get_topk(self._do_ignore_eos(global_scores))
        mapping, self.estimations, best_letters = self._compute_new_beam(best_it)
        self.scores = new_scores.reshape(-1)
        return best_letters.reshape(-1), mapping

    def has_finished(self):
        return all(self.finished_count[i] >= self.beam_size for i in range(self.batch_size))

    def get_graph(self):
        return None

    # ---- pieces shared with the LM-fused searches (:100-145) -------------------
    def to_text(self, est):
        itos = getattr(self, 'itos', None)
        if itos is None:
            return ' '.join(str(int(e)) for e in est)
        return ''.join(itos[e] if itos[e] != '<spc>' else ' ' for e in est)

    def _do_ignore_eos(self, global_scores):
        """(:126-133) ignore EOS from now on; first step: beam 0 only"""
        global_scores = global_scores[:, :-1].contiguous().view(self.batch_size, -1)
        if self.estimations is None:
            global_scores = global_scores[:, :self.num_classes - 1]
        return global_scores

    def _compute_new_beam(self, best_it):
        """(:108-124) with the `batch x beam` loop as two gathers; appends the new
        letters to the re-indexed hypotheses."""
        B, beam, C = self.batch_size, self.beam_size, self.num_classes
        best_beams = best_it // (C - 1)
        best_letters = best_it % (C - 1)
        base = (torch.arange(B, device=best_it.device) * beam)[:, None]
        mapping = (base + best_beams).view(-1)
        if self.estimations is None:
            est = torch.zeros((B * beam, 0), dtype=torch.long, device=best_it.device)
        else:
            est = self.estimations[mapping]
        return mapping, torch.cat((est, best_letters.reshape(-1, 1)), dim=1), best_letters

    def _get_eos_score_from_previous_frame(self, unnormalized_local_scores):
        if self.min_eos is not None:
            unnormalized_local_scores[:, -1] = torch.where(
                unnormalized_local_scores[:, -1] > self.min_eos,
                unnormalized_local_scores[:, -1], self.min_eos)
        self.min_eos = unnormalized_local_scores[:, -1]
        return unnormalized_local_scores

    def _update_eos_scores_with_new_beam(self, beam_mapping):
        self.min_eos = self.min_eos[beam_mapping]


class BeamSearchLM(BeamSearch):
    """Beam search with shallow LM fusion and a coverage term (:185-363); one
    utterance at a time.  A hypothesis carries a bag {LM state: cost}; one step
    pushes the bags of ALL beams through ALL labels in one batched array expansion
    (fst_utils.expand_all_batched) instead of a Python loop over beams x arcs, and
    only the bags of the hypotheses that survive the top-k are turned into dicts."""

    def __init__(self, lm, lm_weight, alphabet_mapping, min_attention_pos,
                 coverage_tau, coverage_weight, *args, **kwargs):
        super(BeamSearchLM, self).__init__(*args, **kwargs)
        self.lm = lm
        self.fst_states = [{self.lm.start(): 0} for _ in range(self.beam_size)]
        self.alphabet_mapping = alphabet_mapping
        self.lm_weight = lm_weight
        self.finished = []
        self.min_attention_pos = min_attention_pos
        self.coverage_tau = coverage_tau
        self.coverage_weight = coverage_weight
        self.best_finished_scores = [float('-inf')] * self.batch_size
        self.best_finished_scores_elements = {'acoustic': [0], 'lm': [0]}
        if self.coverage_weight > 0:
            self.best_finished_scores_elements['coverage'] = [0]
        assert self.batch_size == 1

    class _Bags(object):
        """bags of one step, sorted by bag id = beam * num_classes + LM label"""

        def __init__(self, bag, st, w, num_classes, mapping):
            self.bag, self.st, self.w = bag, st, w
            self.num_classes, self.mapping = num_classes, mapping

        def get(self, beam, letter):
            b = beam * self.num_classes + self.mapping[letter]
            lo, hi = np.searchsorted(self.bag, [b, b + 1])
            return dict(zip(self.st[lo:hi].tolist(), self.w[lo:hi].tolist()))

    def _step_lm(self):
        """(:209-226) -lm_weight * cost of every (beam, letter) extension."""
        C = self.num_classes
        lm_scores = torch.zeros((self.beam_size, C))
        if self.lm_weight == 0:
            return lm_scores, self.fst_states
        sizes = [len(d) for d in self.fst_states]
        grp = np.repeat(np.arange(self.beam_size), sizes)
        st = np.fromiter((k for d in self.fst_states for k in d), np.int64, sum(sizes))
        w = np.fromiter((v for d in self.fst_states for v in d.values()), np.float64, sum(sizes))
        bag, st, w = fst_utils.expand_all_batched(self.lm, C, grp, st, w, True)
        cost = np.full(self.beam_size * C, np.inf)
        if bag.size:
            ub, red = fst_utils._reduce_by_key(bag, w, True)
            cost[ub] = red
        mapping = np.asarray(self.alphabet_mapping, np.int64)
        nxt = np.minimum(1e20, cost.reshape(self.beam_size, C)[:, mapping])
        lm_scores = torch.from_numpy((-self.lm_weight * nxt).astype(np.float32))
        return lm_scores, self._Bags(bag, st, w, C, mapping)

    def _finish_candidates(self, total_scores, att_weights):
        """per-beam (normalised EOS score, may finish) with one host read-back (:236-246)"""
        min_pos = self.min_attention_pos * att_weights.size(0)
        eos = total_scores[:, -1] / (self.estimations.size(1) ** self.length_normalization)
        far = att_weights.argmax(dim=0) > min_pos
        eos_best = torch.argmax(total_scores, dim=1) == total_scores.size(1) - 1
        host = torch.stack([eos, (far & eos_best).to(eos.dtype)]).cpu()
        return host[0], host[1] != 0

    def _set_best(self, score_elements):
        if self.finished[0][0] > self.best_finished_scores[0]:
            self.best_finished_scores[0] = self.finished[0][0]
            self.best_finished[0] = self.finished[0][1]
            self.best_finished_scores_elements = {
                k: [v[self.finished[0][2], -1].item()] for k, v in score_elements.items()}

    def _add_finished(self, total_scores, score_elements, att_weights):
        """(:228-268) hypotheses whose best continuation is EOS, that look far enough
        into the utterance, join the finished list (kept sorted, beam_size long)."""
        eos, ok = self._finish_candidates(total_scores, att_weights)
        finish_mask = [False] * eos.size(0)
        added = False
        for beam in range(eos.size(0)):
            if ok[beam] and eos[beam].item() > -1e10:
                finish_mask[beam] = True
                self.finished += [(eos[beam], self.estimations[beam], beam)]
                added = True
                if self.print_debug:
                    print('Added to finshed {} {}'.format(
                        self.to_text(self.estimations[beam]), eos[beam]))
        if self.finished and added:
            self.finished = sorted(self.finished, key=lambda x: x[0].item(),
                                   reverse=True)[:self.beam_size]
            self._set_best(score_elements)
        return finish_mask

    def _score(self, logits, att_weights):
        """acoustic + LM + coverage scores of every (beam, letter) (:270-310)"""
        if self.coverage_weight > 0:
            if self.coverage is None:
                self.coverage = att_weights.clone()
            else:
                self.coverage += att_weights
        local_scores = logits.squeeze(0)
        if self.keep_eos_score:
            local_scores = self._get_eos_score_from_previous_frame(local_scores)
        local_scores = torch.nn.functional.log_softmax(local_scores, dim=1)
        acoustic_scores = local_scores + self.scores.unsqueeze(1).repeat(1, self.num_classes)
        lm_scores, all_fst_states = self._step_lm()
        lm_scores = lm_scores.to(acoustic_scores.device)
        score_elements = {'acoustic': acoustic_scores.clone(), 'lm': lm_scores.clone()}
        total_scores = acoustic_scores + lm_scores
        if self.coverage_weight > 0:
            coverages = (self.coverage > self.coverage_tau).sum(dim=0).float()
            coverage_scores = self.coverage_weight * coverages.unsqueeze(1).repeat(
                1, self.num_classes)
            total_scores += coverage_scores
            score_elements['coverage'] = coverage_scores
        return acoustic_scores, total_scores, score_elements, all_fst_states

    def _select(self, flat_scores, best_it):
        """(:318-324) scores of the chosen extensions; padding slots are -inf"""
        new_scores = flat_scores[:, best_it[0]]
        if self.beam_size >= flat_scores.size(1):
            new_scores[:, -(self.beam_size - flat_scores.size(1)):] = float('-inf')
        return new_scores.view(-1)

    def _new_fst_states(self, all_fst_states, best_it):
        if self.lm_weight == 0:
            return []
        C = self.num_classes
        return [all_fst_states.get(ind // (C - 1), ind % (C - 1)) for ind in best_it[0].tolist()]

    def _reindex(self, new_beam_mapping):
        if self.keep_eos_score:
            self._update_eos_scores_with_new_beam(new_beam_mapping)
        if self.coverage_weight > 0:
            self.coverage = self.coverage[:, new_beam_mapping]
        if self.attentions is not None:
            self.attentions = self.attentions[:, new_beam_mapping, :]

    def step(self, logits, att_weights, print_lm=None):
        """(:270-356)"""
        if self.gather_attentions:
            if self.attentions is None:
                self.attentions = att_weights.clone().unsqueeze(-1)
            else:
                self.attentions = torch.cat((self.attentions, att_weights.unsqueeze(-1)), dim=-1)
        acoustic_scores, total_scores, score_elements, all_fst_states = self._score(
            logits, att_weights)
        if self.estimations is not None:
            self._add_finished(total_scores, score_elements, att_weights)
        total_scores = self._do_ignore_eos(total_scores)        # ignore EOS from now on
        _, best_it = self._get_topk(total_scores)
        acoustic_scores = acoustic_scores[:, :-1].contiguous().view(self.batch_size, -1)
        self.scores = self._select(acoustic_scores, best_it)
        self.fst_states = self._new_fst_states(all_fst_states, best_it)
        new_beam_mapping, self.estimations, best_letters = self._compute_new_beam(best_it)
        self._reindex(new_beam_mapping)
        if self.print_debug:
            print("%s a:%.3f l:%.f c:%.3f (%d)" % (
                self.to_text(self.estimations[0]), self.scores[0],
                -fst_utils.reduce_weights(self.fst_states[0].values(), True)
                if self.lm_weight > 0 else 0,
                (self.coverage > self.coverage_tau).sum(0)[0].item()
                if self.coverage is not None else 0, len(self.finished)))
        return best_letters.view(-1), new_beam_mapping

    def debug_estimations(self):
        for est in self.estimations:
            print(self.to_text(est))

    def has_finished(self):
        return len(self.finished) >= self.beam_size


class RescoreSearchLM(BeamSearchLM):
    """Forced decoding of a given sentence with the fused score (:366-403)."""

    def __init__(self, sentence, *args, **kwargs):
        super(RescoreSearchLM, self).__init__(*args, **kwargs)
        self.sentence = sentence
        self.gather_attentions = True
        assert self.beam_size == 1

    def _get_topk(self, scores):
        let_id = self.estimations.size(1) if self.estimations is not None else 0
        cur_id = self.sentence[let_id] if let_id < len(self.sentence) else 0
        return (scores[:, cur_id:(cur_id + 1)],
                torch.LongTensor([[cur_id]]).to(scores.device))

    def _add_finished(self, global_scores, score_elements, att_weights):
        if self.estimations.size(1) == len(self.sentence):
            eos = (global_scores[:, -1] /
                   (self.estimations.size(1) ** self.length_normalization)).cpu()
            self.finished += [(eos[0], self.estimations[0], 0)]
            self._set_best(score_elements)


class GraphSearch(BeamSearchLM):
    """BeamSearchLM that merges hypotheses whose recent history (hash_dec), LM
    state set and attention agree, keeping a graph of the merges (:406-648)."""

    def __init__(self, hash_dec, merge_threshold, *args, **kwargs):
        super(GraphSearch, self).__init__(*args, **kwargs)
        self.graph = [{} for _ in range(self.batch_size)]
        self.hash_dec = hash_dec
        self.merge_threshold = merge_threshold

    def att_prod(self, x, y):
        return torch.sum(torch.min(x, y))

    def is_prefix(self, l1, l2):
        if len(l1) > len(l2):
            return False
        return bool((l1 == l2[:len(l1)]).all())

    def step(self, logits, att_weights, print_lm=None):
        """(:424-596)"""
        beam = self.beam_size
        acoustic_scores, total_scores, score_elements, all_fst_states = self._score(
            logits, att_weights)
        if self.estimations is not None:
            finish_mask = self._add_finished(total_scores, score_elements, att_weights)
        else:
            finish_mask = [False] * beam
        if beam > 1 and self.estimations is not None:
            est_host = self.estimations.cpu()
            for beam_id in range(beam):
                if not finish_mask[beam_id]:
                    continue
                li = self.graph[0].get(self.hash_dec(est_host[beam_id]), [])
                for i, (score, atts, (fst, fin, cov), ests, uplink) in enumerate(li):
                    if ests.shape == est_host[beam_id].shape and bool((ests == est_host[beam_id]).all()):
                        li[i] = (score, atts, (fst, True, cov), ests, uplink)

        total_scores = self._do_ignore_eos(total_scores)        # ignore EOS from now on
        _, best_it = self._get_topk(total_scores)
        acoustic_scores = acoustic_scores[:, :-1].contiguous().view(self.batch_size, -1)
        new_scores = self._select(acoustic_scores, best_it)
        new_tot_scores = self._select(total_scores, best_it)
        self.fst_states = new_fst_states = self._new_fst_states(all_fst_states, best_it)
        new_beam_mapping, new_estimations, best_letters = self._compute_new_beam(best_it)
        self.estimations = new_estimations
        self._reindex(new_beam_mapping)

        if beam > 1:
            # the merge bookkeeping runs on host copies (one transfer per step)
            ns, nt = new_scores.cpu(), new_tot_scores.cpu()
            est_host, att_host = new_estimations.cpu(), att_weights.detach().cpu()
            norm = new_estimations.size(1) ** self.length_normalization
            for cur in range(beam):
                if ns[cur] == float('-inf'):
                    continue
                hist_hash = self.hash_dec(est_host[cur])
                li = self.graph[0].get(hist_hash, [])
                new_uplink = None
                for i, (score, atts, (fst, fin, cov), ests, uplink) in enumerate(li):
                    if uplink is not None:
                        continue                                 # dead branch
                    if new_fst_states and set(new_fst_states[cur].keys()) != fst:
                        continue                                 # different LM state
                    if self.att_prod(atts, att_host[:, cur]) < self.merge_threshold:
                        continue                                 # a different branch
                    if score / len(ests) ** self.length_normalization >= nt[cur] / norm:
                        ns[cur] = float('-inf')                  # the old branch is better
                        nt[cur] = float('-inf')
                        new_uplink = i
                        break
                    li[i] = (score, atts, (fst, fin, cov), ests, len(li))
                    for oth in range(beam):                      # drop its descendants
                        if oth != cur and self.is_prefix(ests, est_host[oth]):
                            ns[oth] = float('-inf')
                            nt[oth] = float('-inf')
                # (a VIEW of nt, like the reference's: a branch dropped later in this step reads -inf)
                li.append((nt[cur], att_host[:, cur],
                           (set(new_fst_states[cur].keys()) if new_fst_states else set(),
                            False, None),
                           est_host[cur], new_uplink))
                self.graph[0][hist_hash] = li
            new_scores = ns.to(new_scores.device)
        self.scores = new_scores
        return best_letters.view(-1), new_beam_mapping

    def get_graph(self):
        """(:598-648) vertices (hash, letter, score, coverage, finished) and edges
        (parent hash, hash, 'normal' | 'merged') per utterance."""
        return merge_graphs(self.graph)


def merge_graphs(graph):
    """GraphSearch.get_graph (:598-648) on `graph`, a list over the utterances of
    {hist_hash: [(score, atts, (set_of_states, fin, cov), ests, uplink), ...]}: the one code
    behind the host and the device class.  Uplinks are followed to their sinks in place."""
    for hmap in graph:
        for _, li in hmap.items():
            for i in range(len(li)):
                if li[i][4] is not None:                     # follow uplinks to the sink
                    t = i
                    while li[t][4] is not None:
                        t = li[t][4]
                    li[i] = li[i][:4] + (t,)
            for i in range(len(li)):
                li[i] = li[i][:5] + (hash(tuple(li[i][3].tolist())), li[i][3][-1])
    G = []
    for hmap in graph:
        V = [(hash(()), '<sos>', 0.0, 0., False)]
        valid = {hash(())}
        E = []
        for _, li in hmap.items():
            for sc, atts, (fsts, fin, cov), ests, uplink, ests_hash, label in li:
                if uplink is None:
                    valid.add(ests_hash)
                    V.append((ests_hash, label.item(), sc.item(), cov, fin))
        for _, li in hmap.items():
            for sc, atts, (fsts, fin, cov), ests, uplink, ests_hash, label in li:
                parent = hash(tuple(ests[:-1].tolist()))
                me, kind = ests_hash, 'normal'
                if uplink is not None:
                    me, kind = li[uplink][5], 'merged'
                if parent in valid and me in valid:
                    E.append((parent, me, kind))
        G.append({'V': V, 'E': E})
    return G


def best_result(search):
    """the three keys every `decode` returns, from a search that has finished"""
    return {'decoded': search.best_finished,
            'decoded_scores': search.best_finished_scores_elements,
            'loss': torch.Tensor(search.best_finished_scores).mean()}


def _read_best_finished(search, st):
    """`best_finished` / `best_finished_scores` of a device search from its state arrays `st`"""
    lens = st['best_len'].cpu().tolist()
    toks = st['best_tokens'].cpu().long()
    search.best_finished = [toks[b, :lens[b]] if lens[b] > 0 else []
                            for b in range(search.batch_size)]
    search.best_finished_scores = [float(v) for v in st['best_score'].cpu().tolist()]


class DeviceBeamSearch(object):
    """Plain BeamSearch (reference beam_search.py:13-182) with ALL of its state on the MI355X
    and no host read-back inside a step (`asr_beam_step_f32`): running scores, label
    histories (double-buffered `[B*beam, Lcap]`), per-utterance finished counts and best
    finished hypotheses.  `step` only enqueues a launch; `poll_finished` reads the
    device-side flag (the caller decides how often); `finalize` copies the results into the
    attributes the reference's object exposes (`finished_count`, `best_finished`,
    `best_finished_scores`, `best_finished_scores_elements`, `estimations`, `scores`)."""

    def __init__(self, batch_size, beam_size, device, num_classes, length_normalization,
                 max_steps):
        from att_speech import _native
        self._native = _native
        self.batch_size, self.beam_size, self.num_classes = batch_size, beam_size, num_classes
        self.length_normalization = length_normalization
        hyps, cap = batch_size * beam_size, max_steps + 1
        i32 = dict(dtype=torch.int32, device=device)
        self._scores = [torch.zeros(hyps, device=device), torch.zeros(hyps, device=device)]
        self._est = [torch.zeros((hyps, cap), **i32), torch.zeros((hyps, cap), **i32)]
        self._state = {
            'finished_count': torch.zeros(batch_size, **i32),
            'best_score': torch.full((batch_size,), float('-inf'), device=device),
            'best_len': torch.zeros(batch_size, **i32),
            'best_tokens': torch.zeros((batch_size, cap), **i32),
            'new_input': torch.zeros(hyps, **i32), 'parent': torch.zeros(hyps, **i32),
            'done': torch.zeros(3, **i32)}
        self._step = 0
        self.coverage = None
        self.print_debug = False
        self.estimations = None
        self.scores = self._scores[0]

    def step(self, logits, *args, **kwargs):
        """logits [1, B*beam, C] or [B*beam, C] -> (chosen labels, parent hypothesis) as
        int32 device tensors (valid until the next step)."""
        s = self._step
        logits = logits.reshape(-1, self.num_classes).contiguous()
        len_div = float(s ** self.length_normalization) if s > 0 else 1.0
        self._native.beam_step(logits, self._scores[s & 1], self._scores[(s + 1) & 1],
                               self._est[s & 1], self._est[(s + 1) & 1], s, self.batch_size,
                               self.beam_size, len_div, self._state)
        self._step = s + 1
        return self._state['new_input'], self._state['parent']

    def poll_finished(self):
        return bool(int(self._state['done'][0].item()))

    has_finished = poll_finished

    def get_graph(self):
        return None

    def finalize(self):
        st = self._state
        done = st['done'].cpu().tolist()
        eff = int(done[2])                       # steps that took effect
        self.finished_count = st['finished_count'].cpu().tolist()
        _read_best_finished(self, st)
        self.best_finished_scores_elements = {'acoustic': self.best_finished_scores}
        self.estimations = self._est[eff & 1][:, :eff].long()
        self.scores = self._scores[eff & 1]
        return self


class DeviceBeamSearchLM(object):
    """BeamSearchLM (reference beam_search.py:185-363) with ALL of its state on the MI355X, for any
    number of utterances: B utterances behave as B independent BeamSearchLM(batch_size=1) runs,
    each on its own `enc_lens[b]` encoder frames (the own length stands where the host class
    reads `att_weights.size(0)`).  Per label step: `asr_lm_label_costs_f64` (LM cost of every
    extension from the bags, fp64), `asr_beam_lm_step_f32` (scores, finish test, finished list,
    best hypothesis, top-k, re-indexing, freeze) and `asr_lm_bag_advance_f64` (the survivors'
    bags) — no host read-back.  An utterance whose finished list reached `beam_size` is frozen:
    later launches change nothing of it.  `poll_finished` reads the frozen flags and the
    bag-overflow word in one copy; `finalize` fills the attributes of the host class, each with
    one entry per utterance (`finished`, `estimations`, `scores`, `coverage`, `fst_states` are
    lists over the utterances).

    Quirk of the host class kept on purpose: `best_finished_scores_elements` holds THIS step's
    score elements (EOS column) at the beam index stored with `finished[0]`, which may have
    joined the list steps ago, when that beam index meant another hypothesis."""

    def __init__(self, lm, lm_weight, alphabet_mapping, min_attention_pos, coverage_tau,
                 coverage_weight, batch_size, beam_size, device, num_classes, length_normalization,
                 max_steps, max_frames, enc_lens, keep_eos_score=False):
        from att_speech import _native
        self._native = _native
        self.lm, self.lm_weight = lm, float(lm_weight)
        self.batch_size, self.beam_size, self.num_classes = batch_size, beam_size, num_classes
        self.length_normalization = length_normalization
        self.min_attention_pos = float(min_attention_pos)
        self.coverage_tau, self.coverage_weight = float(coverage_tau), float(coverage_weight)
        self.keep_eos_score = keep_eos_score
        B, beam, cap, T = batch_size, beam_size, max_steps + 1, max_frames
        hyps, bc = B * beam, _native.LM_BAG_CAP
        z = self._z = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
        zi = self._zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)  # noqa: E731
        self._lens = torch.as_tensor(enc_lens).to(device, torch.int32).contiguous()
        self._scores = [z(hyps), z(hyps)]
        self._est = [zi(hyps, cap), zi(hyps, cap)]
        self._cov = [z(hyps, T), z(hyps, T)] if self.coverage_weight > 0 else [None, None]
        self._min_eos = torch.full((hyps,), float('-inf'), device=device) if keep_eos_score else None
        self._use_lm = self.lm_weight != 0
        self._lmdev = self._mapping = self._cost = None
        self._bags = [None, None]
        if self._use_lm:
            self._lmdev = lm.device_arrays(device)
            self._mapping = torch.as_tensor(list(alphabet_mapping)).to(device, torch.int32).contiguous()
            self._cost = torch.zeros(hyps, num_classes, dtype=torch.float64, device=device)
            for k in range(2):
                self._bags[k] = (zi(hyps, bc), torch.zeros(hyps, bc, dtype=torch.float64, device=device),
                                 zi(hyps))
            self._bags[0][0][:, 0] = lm.start()         # every hypothesis starts as {start: 0}
            self._bags[0][2][:] = 1
        self._state = {
            'fin_count': zi(B), 'fin_parity': zi(B), 'fin_score': z(2, B, beam),
            'fin_len': zi(2, B, beam), 'fin_beam': zi(2, B, beam), 'fin_tokens': zi(2, B, beam, cap),
            'best_score': torch.full((B,), float('-inf'), device=device), 'best_len': zi(B),
            'best_tokens': zi(B, cap), 'best_elems': z(B, 3),
            'new_input': zi(hyps), 'parent': zi(hyps),
            # frozen [B] and the bag-overflow word behind it: one copy per poll
            'flags': zi(B + 1), 'nsteps': zi(B)}
        self._state['frozen'] = self._state['flags'][:B]
        self._state['overflow'] = self._state['flags'][B:]
        self._step = 0
        self._step_outputs = ()         # a subclass's (fin_mask, tot_out): the graph step entry
        self.overflow = 0
        self.print_debug = False
        self.estimations = None
        self.coverage = None

    def step(self, logits, att_weights, *args, **kwargs):
        """logits [1, B*beam, C] or [B*beam, C]; att_weights [B*beam, T], this step's alignment ->
        (chosen labels, parent hypothesis) as int32 device tensors (valid until the next step)."""
        s, n, st = self._step, self._native, self._state
        B, beam = self.batch_size, self.beam_size
        logits = logits.reshape(-1, self.num_classes).contiguous()
        att = att_weights.contiguous()
        len_div = float(s ** self.length_normalization) if s > 0 else 1.0
        i, o = s & 1, (s + 1) & 1
        if self._use_lm:
            n.lm_label_costs(self._lmdev, *self._bags[i], self._mapping, st['frozen'], B, beam,
                             self.num_classes, self._cost)
        n.beam_lm_step(logits, att, self._lens, self._cost, self.lm_weight, self._scores[i],
                       self._scores[o], self._est[i], self._est[o], self._cov[i], self._cov[o],
                       self._min_eos, s, B, beam, len_div, self.min_attention_pos, self.coverage_tau,
                       self.coverage_weight, st, *self._step_outputs)
        if self._use_lm:
            n.lm_bag_advance(self._lmdev, self._mapping, self._bags[i], self._bags[o], st['parent'],
                             st['new_input'], st['nsteps'], s, B, beam, st['overflow'])
        self._after_advance(att, s)
        self._step = s + 1
        return st['new_input'], st['parent']

    def _after_advance(self, att, s):
        """what a subclass enqueues behind the step of label position `s`, once the bags advanced"""

    def poll_finished(self):
        """True when every utterance is frozen or a bag overflowed (`self.overflow` = its size)."""
        flags = self._state['flags'].cpu().tolist()
        self.overflow = int(flags[-1])
        return self.overflow > 0 or all(flags[:-1])

    has_finished = poll_finished

    def get_graph(self):
        return None

    def finalize(self):
        st = {k: v.cpu() for k, v in self._state.items()}
        B, beam = self.batch_size, self.beam_size
        self.overflow = int(st['overflow'][0])
        eff = st['nsteps'].tolist()                  # steps that took effect, per utterance
        _read_best_finished(self, st)
        el = st['best_elems'].tolist()
        self.best_finished_scores_elements = {'acoustic': [el[b][0] for b in range(B)],
                                              'lm': [el[b][1] for b in range(B)]}
        if self.coverage_weight > 0:
            self.best_finished_scores_elements['coverage'] = [el[b][2] for b in range(B)]
        par = st['fin_parity'].tolist()
        self.finished = []
        for b in range(B):
            n = int(st['fin_count'][b])
            self.finished.append([
                (st['fin_score'][par[b], b, r],
                 st['fin_tokens'][par[b], b, r, :int(st['fin_len'][par[b], b, r])].long(),
                 int(st['fin_beam'][par[b], b, r])) for r in range(n)])
        sl = lambda t, b: t[b * beam:(b + 1) * beam]  # noqa: E731
        est = [e.cpu() for e in self._est]
        sc = [s.cpu() for s in self._scores]
        self.estimations = [sl(est[eff[b] & 1], b)[:, :eff[b]].long() for b in range(B)]
        self.scores = [sl(sc[eff[b] & 1], b) for b in range(B)]
        self.coverage = None
        if self.coverage_weight > 0:
            cov = [c.cpu() for c in self._cov]
            ln = self._lens.cpu().tolist()
            self.coverage = [sl(cov[eff[b] & 1], b)[:, :ln[b]].t() for b in range(B)]
        self.fst_states = []
        if self._use_lm:
            bags = [[t.cpu() for t in bg] for bg in self._bags]
            for b in range(B):
                bs, bw, bn = bags[eff[b] & 1]
                self.fst_states.append([
                    dict(zip(bs[h, :int(bn[h])].tolist(), bw[h, :int(bn[h])].tolist()))
                    for h in range(b * beam, (b + 1) * beam)])
        else:
            self.fst_states = [[] for _ in range(B)]
        return self


# The node store of DeviceGraphSearch is refused above this many bytes (checked before anything
# is allocated): the caller decodes on the host instead, one utterance at a time.
GRAPH_STORE_BUDGET_BYTES = 2 << 30


class GraphStoreOverBudget(MemoryError):
    """what DeviceGraphSearch raises in place of allocating such a store; carries both figures"""

    def __init__(self, need, budget):
        super(GraphStoreOverBudget, self).__init__(
            'a node store of %d bytes is above the budget of %d' % (need, budget))
        self.need, self.budget = need, budget


class DeviceGraphSearch(DeviceBeamSearchLM):
    """GraphSearch (reference beam_search.py:406-648) on the MI355X for any number of utterances: B
    utterances behave as B independent GraphSearch(batch_size=1) runs.  Per label step
    `asr_lm_label_costs_f64`, `asr_beam_lm_step_graph_f32` (the BeamSearchLM step plus the finish
    mask and the fused scores of the survivors), `asr_lm_bag_advance_f64` and `asr_graph_merge_f32`
    (the merge bookkeeping on a per-utterance node store of max_steps * beam nodes, which every
    step's slots fit by construction).  With beam 1 the merge launch is skipped and the graph
    stays empty, as on the host.  `span` is the number of labels of the merge key (hash_dec's);
    labels are compared directly, so collisions of Python's hash() between different keys are not
    reproduced.  `finalize` rebuilds `self.graph` in the host's layout, a list over the utterances
    of {hist_hash: [(score, atts, (set_of_states, fin, None), ests, uplink), ...]} with buckets
    in insertion order and bucket-local uplinks; `get_graph` is the host's code."""

    def __init__(self, hash_dec, merge_threshold, span, lm, lm_weight, alphabet_mapping,
                 min_attention_pos, coverage_tau, coverage_weight, batch_size, beam_size, device,
                 num_classes, length_normalization, max_steps, max_frames, enc_lens,
                 keep_eos_score=False):
        need = self.store_bytes(batch_size, beam_size, max_steps, max_frames)
        if need > GRAPH_STORE_BUDGET_BYTES:              # the one check, before anything is allocated
            raise GraphStoreOverBudget(need, GRAPH_STORE_BUDGET_BYTES)
        super(DeviceGraphSearch, self).__init__(
            lm, lm_weight, alphabet_mapping, min_attention_pos, coverage_tau, coverage_weight,
            batch_size, beam_size, device, num_classes, length_normalization, max_steps, max_frames,
            enc_lens, keep_eos_score=keep_eos_score)
        self.hash_dec, self.merge_threshold, self.span = hash_dec, float(merge_threshold), int(span)
        B, beam, cap, T = batch_size, beam_size, max_steps + 1, max_frames
        ncap, bc = max_steps * beam, self._native.LM_BAG_CAP
        z, zi = self._z, self._zi
        self._fin_mask, self._tot = zi(B * beam), z(B * beam)
        self._step_outputs = (self._fin_mask, self._tot)
        self._len_pow = torch.tensor([float(l ** length_normalization) for l in range(cap + 1)],
                                     dtype=torch.float32, device=device)
        self._store = {
            'node_count': zi(B), 'node_score': z(B, ncap),
            'node_len': zi(B, ncap), 'node_tokens': zi(B, ncap, cap),
            'node_att': z(B, ncap, T), 'node_bag_n': zi(B, ncap),
            'node_bag_state': zi(B, ncap, bc), 'node_fin': zi(B, ncap),
            'node_uplink': torch.full((B, ncap), -1, dtype=torch.int32, device=device)}
        self.graph = [{} for _ in range(B)]

    @staticmethod
    def store_bytes(batch_size, beam_size, max_steps, max_frames):
        from att_speech import _native
        per_node = 4 * (5 + (max_steps + 1) + max_frames + _native.LM_BAG_CAP)
        return batch_size * (4 + max_steps * beam_size * per_node)

    def step(self, logits, att_weights, *args, **kwargs):
        """DeviceBeamSearchLM's step through the graph entry (`_step_outputs`), then the merge."""
        assert (self._step + 1) * self.beam_size <= self._store['node_score'].shape[1]   # the store cannot overflow
        return super(DeviceGraphSearch, self).step(logits, att_weights)

    def _after_advance(self, att, s):
        B, beam, i, o = self.batch_size, self.beam_size, s & 1, (s + 1) & 1
        if beam > 1:
            self._native.graph_merge(
                att, self._lens, self._scores[o], self._tot, self._est[i], self._est[o],
                self._fin_mask, self._bags[o] if self._use_lm else None, self._state['nsteps'],
                self._len_pow, s, B, beam, self.span, self.merge_threshold, self._store)

    def finalize(self):
        super(DeviceGraphSearch, self).finalize()
        store = {k: v.cpu() for k, v in self._store.items()}
        lens = self._lens.cpu().tolist()
        self.graph = []
        for b in range(self.batch_size):
            hmap, local, buckets = {}, [], []
            for i in range(int(store['node_count'][b])):
                ests = store['node_tokens'][b, i, :int(store['node_len'][b, i])].long()
                nb = int(store['node_bag_n'][b, i])
                li = hmap.setdefault(self.hash_dec(ests), [])
                up = int(store['node_uplink'][b, i])
                local.append(len(li))
                buckets.append(li)
                li.append((store['node_score'][b, i], store['node_att'][b, i, :lens[b]],
                           (set(store['node_bag_state'][b, i, :nb].tolist()),
                            bool(store['node_fin'][b, i]), None), ests, None if up < 0 else up))
            # node indices -> bucket-local ones (an uplink may point at a node appended later)
            for i, li in enumerate(buckets):
                e = li[local[i]]
                if e[4] is not None:
                    li[local[i]] = e[:4] + (local[e[4]],)
            self.graph.append(hmap)
        return self

    def get_graph(self):
        return merge_graphs(self.graph)


# ---------------------------------------------------------------------------------------------
# Forced scoring of given sentences (the reference's egs/wsj/local/lattice_search scripts)
# ---------------------------------------------------------------------------------------------
def graph_sentences(graph, limit=None):
    """The label-id sentences of every path from the root to a finished node of `graph`, one
    {'V': [(hash, label, score, coverage, finished), ...], 'E': [(parent, child, kind), ...]} as
    `decode` returns per utterance (get_graph / merge_graphs; V[0] is the root): the `dfs` of
    rescore_lattices2.py, iteratively and over label ids instead of characters.  A node's sentence
    comes before those of its children, children in edge order; a node reached along several paths
    yields one sentence per path.  Stops after `limit` sentences.  An edge back to a node of the
    current path is not followed (the script's recursion would not end on it)."""
    if limit is not None and limit <= 0:
        return []
    nodes = {v[0]: v for v in graph['V']}               # a repeated hash keeps its last entry
    children = {h: [] for h in nodes}
    for edge in graph['E']:
        children[edge[0]].append(edge[1])
    root = graph['V'][0][0]
    out, path, on_path = [], [], {root}
    if nodes[root][4]:
        out.append([])
    stack = [(root, iter(children[root]))]
    while stack and (limit is None or len(out) < limit):
        node, it = stack[-1]
        nxt = next(it, None)
        if nxt is None:
            stack.pop()
            on_path.discard(node)
            if path:
                path.pop()
            continue
        if nxt in on_path:
            continue
        path.append(int(nodes[nxt][1]))
        on_path.add(nxt)
        if nodes[nxt][4]:
            out.append(list(path))
        stack.append((nxt, iter(children[nxt])))
    return out


def sentence_trie(sentences, eos):
    """The prefix trie of one utterance's sentences (lists of labels, no EOS), level by level.
    Returns {'inverse': distinct-sentence id of every given sentence, 'count': number of distinct
    sentences, 'lengths': their lengths (without EOS), 'levels': [...]}; level l describes its
    units, the distinct prefixes of length l that a sentence extends (by a label or by EOS):
    `parent` (unit of level l-1; empty at level 0), `label` (the last label), and the outgoing edges
    in CSR form, `edge_ptr` / `edge_label` / `edge_dst` with edge_dst >= 0 the unit of level l+1
    the edge creates and -1 - s for the EOS edge of distinct sentence s.  Built by one row sort of
    the padded sentence matrix and one pass of array operations per level."""
    n_given = len(sentences)
    lens = np.fromiter((len(s) for s in sentences), np.int64, n_given)
    if n_given == 0:
        return {'inverse': np.zeros(0, np.int64), 'count': 0, 'lengths': lens, 'levels': []}
    width = int(lens.max()) + 1
    mat = np.full((n_given, width), -1, np.int64)
    flat = np.fromiter((c for s in sentences for c in s), np.int64, int(lens.sum()))
    cols = np.arange(width)[None, :]
    mat[cols < lens[:, None]] = flat
    mat[np.arange(n_given), lens] = eos
    mat, inverse = np.unique(mat, axis=0, return_inverse=True)       # rows in lexicographic order
    inverse = np.asarray(inverse).reshape(-1)
    m = mat.shape[0]
    n = (mat >= 0).sum(1) - 1                                        # lengths without EOS
    # differs[i, l]: row i and row i-1 differ somewhere in their first l columns
    differs = np.ones((m, width + 1), bool)
    differs[1:, 0] = False
    differs[1:, 1:] = np.logical_or.accumulate(mat[1:] != mat[:-1], axis=1)
    levels, unit_prev, prev = [], None, None
    for l in range(int(n.max()) + 1):
        active = np.nonzero(n >= l)[0]              # rows sharing a prefix of length l are adjacent
        first = differs[active, l]
        unit = np.full(m, -1, np.int64)
        unit[active] = np.cumsum(first) - 1
        heads = active[first]
        level = {'n_units': int(first.sum()),
                 'parent': unit_prev[heads] if l else np.zeros(0, np.int64),
                 'label': mat[heads, l - 1] if l else np.zeros(0, np.int64)}
        ends = active[n[active] == l]               # the sentences that end here: their EOS edges
        level['_eos'] = (unit[ends], ends)
        if prev is not None:
            _close_level(prev, level, eos)
        levels.append(level)
        unit_prev, prev = unit, level
    _close_level(prev, None, eos)
    return {'inverse': inverse, 'count': m, 'lengths': n, 'levels': levels}


def _close_level(level, nxt, eos):
    """the CSR edge lists of `level` once the units of the next level are known"""
    src_eos, sent = level.pop('_eos')
    src = [src_eos, nxt['parent']] if nxt is not None else [src_eos]
    lab = [np.full(len(sent), eos, np.int64)] + ([nxt['label']] if nxt is not None else [])
    dst = [-1 - sent] + ([np.arange(nxt['n_units'])] if nxt is not None else [])
    src, lab, dst = np.concatenate(src), np.concatenate(lab), np.concatenate(dst)
    order = np.argsort(src, kind='stable')
    level['edge_ptr'] = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=level['n_units']))))
    level['edge_label'], level['edge_dst'] = lab[order], dst[order]


def batch_trie_levels(tries):
    """The per-utterance tries of one call side by side: level l is as wide as the widest utterance
    at that level, slot = utterance * width + unit; surplus slots are dead (they continue slot 0 of
    their utterance and have no edges).  Sentence ids become global (offset by the distinct
    sentences of the utterances before).  Returns (levels, sentence offsets); every level holds
    `width`, `parent` / `label` [B * width] (parent indexes the previous level's slots; at level 0
    the utterance), `edge_ptr` [B * width + 1], `edge_label` / `edge_dst` [edges] (global slots of
    the next level, or -1 - global sentence) and `edge_src` [edges], the slot of every edge."""
    B = len(tries)
    offsets = np.concatenate(([0], np.cumsum([t['count'] for t in tries]))).astype(np.int64)
    depth = max([len(t['levels']) for t in tries] + [0])
    widths = [max([t['levels'][l]['n_units'] for t in tries if l < len(t['levels'])] + [1])
              for l in range(depth)]
    out = []
    for l in range(depth):
        W, Wp, Wn = widths[l], (widths[l - 1] if l else 1), (widths[l + 1] if l + 1 < depth else 1)
        parent = np.repeat(np.arange(B) * Wp, W)                      # dead: slot 0 of the utterance
        label = np.zeros(B * W, np.int64)
        counts = np.zeros(B * W, np.int64)
        e_lab, e_dst = [], []
        for u, t in enumerate(tries):
            if l >= len(t['levels']):
                continue
            lv = t['levels'][l]
            k = lv['n_units']
            if l:
                parent[u * W:u * W + k] = u * Wp + lv['parent']
                label[u * W:u * W + k] = lv['label']
            counts[u * W:u * W + k] = np.diff(lv['edge_ptr'])
            d = lv['edge_dst']
            e_lab.append(lv['edge_label'])
            e_dst.append(np.where(d >= 0, d + u * Wn, d - offsets[u]))
        e_lab = np.concatenate(e_lab) if e_lab else np.zeros(0, np.int64)
        e_dst = np.concatenate(e_dst) if e_dst else np.zeros(0, np.int64)
        out.append({'width': W, 'parent': parent, 'label': label,
                    'edge_ptr': np.concatenate(([0], np.cumsum(counts))),
                    'edge_label': e_lab, 'edge_dst': e_dst,
                    'edge_src': np.repeat(np.arange(B * W), counts)})
    return out, offsets


class DeviceForcedScorer(object):
    """The bookkeeping of `AttentionDecoderTCN.score_sentences` on the MI355X: per trie level one
    `asr_forced_level_f32` launch (coverage rows, log-partition, the fp64 acoustic carries, the
    finished sentences' sums and covered-frame counts) and, with an LM, one
    `asr_lm_bag_advance_f64` over the level's edges (one bag per edge row; a unit's bag is the row
    of the edge that created it) followed by -logsumexp(-cost) of the EOS rows in fp64.  Every index
    array of every level is uploaded once, before the first launch; `finish` reads everything back
    in one copy.  Buffers are as wide as the widest level."""

    def __init__(self, levels, n_sent, batch_size, device, num_classes, max_frames, enc_lens,
                 coverage_tau, lm=None, alphabet_mapping=None):
        from att_speech import _native
        self._native = _native
        self.levels, self.n_sent, self.batch_size = levels, int(n_sent), batch_size
        self.num_classes, self.coverage_tau = num_classes, float(coverage_tau)
        self._lens = torch.as_tensor(enc_lens).to(device, torch.int32).contiguous()
        slots = max(batch_size * lv['width'] for lv in levels)
        rows = max(max(len(lv['edge_label']) for lv in levels), 1)
        self.rows = rows
        self._use_lm = lm is not None
        # ---- one upload of every level's indices (int32 for the launches, int64 for torch) ----
        parts, self._where = [], []
        at = 0
        for l, lv in enumerate(levels):
            arrays = {k: lv[k] for k in ('parent', 'label', 'edge_ptr', 'edge_label', 'edge_dst')}
            eos = np.nonzero(lv['edge_dst'] < 0)[0]
            arrays['eos_rows'], arrays['eos_sent'] = eos, -1 - lv['edge_dst'][eos]
            if self._use_lm:
                # the bag of a slot: row 0 (the start bag) at level 0, else the row of its edge
                bag_row = np.zeros(batch_size * lv['width'], np.int64)
                if l:
                    made = np.nonzero(levels[l - 1]['edge_dst'] >= 0)[0]
                    bag_row[levels[l - 1]['edge_dst'][made]] = made
                adv_parent = np.zeros(rows, np.int64)
                adv_input = np.full(rows, -1, np.int64)            # surplus rows: left alone
                adv_parent[:len(lv['edge_src'])] = bag_row[lv['edge_src']]
                adv_input[:len(lv['edge_label'])] = lv['edge_label']
                arrays['adv_parent'], arrays['adv_input'] = adv_parent, adv_input
            where = {}
            for k, a in arrays.items():
                where[k] = (at, at + len(a))
                parts.append(np.asarray(a, np.int64))
                at += len(a)
            self._where.append(where)
        host = np.concatenate(parts)
        self._i64 = torch.from_numpy(host).to(device)
        self._i32 = self._i64.to(torch.int32)
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self._cov = [torch.zeros(slots, max_frames, device=device) for _ in range(2)]
        self._ac = [torch.zeros(slots, **f64) for _ in range(2)]
        self._sent = torch.zeros(3, max(self.n_sent, 1), **f64)       # acoustic, lm cost, covered
        self._sent_cov = torch.zeros(max(self.n_sent, 1), **i32)
        self._overflow = torch.zeros(1, **i32)
        if self._use_lm:
            bc = _native.LM_BAG_CAP
            self._lmdev = lm.device_arrays(device)
            self._mapping = torch.as_tensor(list(alphabet_mapping)).to(device, torch.int32).contiguous()
            self._bags = [(torch.zeros(rows, bc, **i32), torch.zeros(rows, bc, **f64),
                           torch.zeros(rows, **i32)) for _ in range(2)]
            self._bags[0][0][0, 0] = lm.start()                       # row 0 = {start: 0}
            self._bags[0][2][0] = 1
            self._nsteps = torch.zeros(1, **i32)
            self._slot = torch.arange(bc, device=device)[None, :]
        self._level = 0

    def index(self, l, key, long=False):
        lo, hi = self._where[l][key]
        return (self._i64 if long else self._i32)[lo:hi]

    def step(self, logits, att, att_init=None):
        """logits [B * width, C], att [B * width, T] of this level (att_init [B, T]: the initial
        alignments, level 0 only).  Enqueues the launches of the level; nothing is read back."""
        l, n = self._level, self._native
        lv = self.levels[l]
        i, o = l & 1, (l + 1) & 1
        cov_in = att_init if l == 0 else self._cov[i]
        n.forced_level(logits.reshape(-1, self.num_classes).contiguous(), att.contiguous(), cov_in,
                       self._cov[o], self.index(l, 'parent'), self.index(l, 'edge_ptr'),
                       self.index(l, 'edge_label'), self.index(l, 'edge_dst'), self._ac[i],
                       self._ac[o], self._lens, self.batch_size, lv['width'], self.coverage_tau,
                       self._sent[0], self._sent_cov)
        if self._use_lm:
            self._nsteps.add_(1)
            n.lm_bag_advance(self._lmdev, self._mapping, self._bags[i], self._bags[o],
                             self.index(l, 'adv_parent'), self.index(l, 'adv_input'), self._nsteps,
                             l, 1, self.rows, self._overflow)
            rows = self.index(l, 'eos_rows', long=True)
            if rows.numel():
                cost = self._bags[o][1].index_select(0, rows)
                live = self._slot < self._bags[o][2].index_select(0, rows)[:, None]
                neg = torch.where(live, -cost, torch.full_like(cost, float('-inf')))
                self._sent[1].index_copy_(0, self.index(l, 'eos_sent', long=True),
                                          -torch.logsumexp(neg, 1))
        self._level = l + 1

    def finish(self):
        """-> (acoustic [n_sent] fp64, covered [n_sent] int64, lm cost [n_sent] fp64 or None,
        overflow): the one read-back of the call."""
        self._sent[2].copy_(self._sent_cov)
        host = torch.cat((self._sent.reshape(-1), self._overflow.double())).cpu().numpy()
        self.overflow = int(host[-1])
        vals = host[:-1].reshape(3, -1)[:, :self.n_sent]
        return (vals[0], vals[2].astype(np.int64), vals[1] if self._use_lm else None,
                self.overflow)
