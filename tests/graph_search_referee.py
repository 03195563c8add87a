"""fp64 referee of the merge launch of the device graph search (asr_graph_merge_f32) and of the two
extra outputs of asr_beam_lm_step_graph_f32 (include/asr_amd.h).  Written from the host class
(modules/beam_search.py, GraphSearch.step), not from the kernel: plain numpy on the CPU, Python
loops over lists of nodes, no native calls.

`merge_ref` returns the wanted node store and scores, the margin of every decision it took
(`min_sum`: |min-sum - threshold|; `score`: |old / len^ln - new / len^ln|, finite operands only) and
counts of what happened (`events`), so that a test can tell it did not pass vacuously.  `mut` plants
one wrong term (MUTANTS) for tests/test_graph_search_referee.py.  `RefGraphSearch` chains it behind
lm_beam_referee's step."""
import collections

import numpy as np

import lm_beam_referee as lr

INF = float('inf')
POISON = lr.POISON
BAG_CAP = lr.BAG_CAP
MUTANTS = ('parent_column', 'gt_for_ge', 'no_alias_rewrite', 'dead_nodes_not_skipped',
           'descendants_not_dropped', 'lm_state_test_skipped', 'finished_mark_skipped')
NODE_KEYS = ('node_count', 'node_score', 'node_len', 'node_tokens', 'node_att', 'node_bag_n',
             'node_bag_state', 'node_fin', 'node_uplink')


def fresh_store(B, Ncap, Lcap, T, poison=False):
    """an empty node store; poison=True fills everything but the counts as a launch must not read it"""
    st = dict(node_count=np.zeros(B, np.int32), node_score=np.zeros((B, Ncap), np.float32),
              node_len=np.zeros((B, Ncap), np.int32), node_tokens=np.zeros((B, Ncap, Lcap), np.int32),
              node_att=np.zeros((B, Ncap, T), np.float32), node_bag_n=np.zeros((B, Ncap), np.int32),
              node_bag_state=np.zeros((B, Ncap, BAG_CAP), np.int32), node_fin=np.zeros((B, Ncap), np.int32),
              node_uplink=np.full((B, Ncap), -1, np.int32))
    if poison:
        for k, v in st.items():
            if k != 'node_count':
                v[...] = np.nan if v.dtype.kind == 'f' else POISON
    return st


def key_of(tokens, span):
    """hash_dec's tuple: the last `span` labels, left-filled with -1 (span 0: one bucket)"""
    if span == 0:
        return ()
    tail = [int(v) for v in tokens[-span:]]
    return tuple([-1] * (span - len(tail)) + tail)


def len_pow(Lcap, ln):
    return np.array([float(l ** ln) for l in range(Lcap + 1)], np.float32)


def merge_ref(c, mut=None):
    """One asr_graph_merge_f32 launch.  c: att [hyps, T], lens [B], scores / tot [hyps] (the step
    entry's scores_out / tot_out), est_in / est_out [hyps, Lcap], fin_mask [hyps], bags (list of dicts
    in ascending state order, the survivors'; None: no LM term), nsteps [B], parent [hyps] (for the
    mutant only), step, B, beam, span, merge_threshold, length_normalization, store (not modified).
    -> (out, margins, events); out: the store's arrays after the launch (node_score fp64), scores, tot."""
    B, beam, step, span = c['B'], c['beam'], c['step'], c['span']
    thr, ln = float(c['merge_threshold']), c['length_normalization']
    L = step + 1
    st = {k: np.array(c['store'][k], copy=True) for k in NODE_KEYS}
    st['node_score'] = st['node_score'].astype(np.float64)
    att = np.asarray(c['att'], np.float64)
    scores = np.array(c['scores'], np.float64)
    tot = np.array(c['tot'], np.float64)
    est_in, est_out = np.asarray(c['est_in']), np.asarray(c['est_out'])
    m = dict(min_sum=INF, score=INF)
    ev = collections.Counter()
    for b in range(B):
        if int(c['nsteps'][b]) != L:
            continue                                             # frozen before this step
        h0, tlen = b * beam, int(c['lens'][b])
        cnt = int(st['node_count'][b])
        seq = lambda i: st['node_tokens'][b, i, :st['node_len'][b, i]]  # noqa: E731
        if step > 0 and mut != 'finished_mark_skipped':
            for k in range(beam):
                if not c['fin_mask'][h0 + k]:
                    continue
                hist = est_in[h0 + k, :step]
                for i in range(cnt):
                    if st['node_len'][b, i] == step and np.array_equal(seq(i), hist):
                        st['node_fin'][b, i] = 1
                        ev['finished_marks'] += 1
        slot_node = {}
        for cur in range(beam):
            h = h0 + cur
            if scores[h] == -INF:
                ev['dead_slots'] += 1
                continue
            hist = est_out[h, :L]
            key = key_of(hist, span)
            states = None if c['bags'] is None else sorted(c['bags'][h])
            col = att[int(c['parent'][h])] if mut == 'parent_column' else att[h]
            new_uplink = -1
            tried = 0
            for i in range(cnt):                                 # (nodes appended for `cur` come after the walk)
                if key_of(seq(i), span) != key:
                    continue
                tried += 1
                if st['node_uplink'][b, i] >= 0 and mut != 'dead_nodes_not_skipped':
                    ev['dead_candidates'] += 1
                    continue
                if states is not None and mut != 'lm_state_test_skipped':
                    if st['node_bag_state'][b, i, :st['node_bag_n'][b, i]].tolist() != states:
                        ev['lm_state_mismatches'] += 1
                        continue
                s = float(np.minimum(st['node_att'][b, i, :tlen].astype(np.float64), col[:tlen]).sum())
                m['min_sum'] = min(m['min_sum'], abs(s - thr))
                if s < thr:
                    ev['below_threshold'] += 1
                    continue
                nl = int(st['node_len'][b, i])
                with np.errstate(divide='ignore', invalid='ignore'):
                    old = st['node_score'][b, i] / np.float64(nl) ** ln
                    new = tot[h] / np.float64(L) ** ln
                if np.isfinite(old) and np.isfinite(new):
                    m['score'] = min(m['score'], abs(old - new))
                    ev['ties'] += int(old == new)
                if (old > new) if mut == 'gt_for_ge' else (old >= new):
                    scores[h] = tot[h] = -INF                    # the old branch is better
                    new_uplink = i
                    ev['old_wins'] += 1
                    break
                st['node_uplink'][b, i] = cnt                    # the new branch wins
                ev['new_wins'] += 1
                if mut == 'descendants_not_dropped':
                    continue
                cand = seq(i)
                for oth in range(beam):
                    if oth != cur and len(cand) <= L and np.array_equal(cand, est_out[h0 + oth, :len(cand)]):
                        if scores[h0 + oth] != -INF:
                            ev['drops'] += 1
                        scores[h0 + oth] = tot[h0 + oth] = -INF
                        if oth in slot_node and mut != 'no_alias_rewrite':
                            if st['node_score'][b, slot_node[oth]] != -INF:
                                ev['alias_rewrites'] += 1
                            st['node_score'][b, slot_node[oth]] = -INF       # the host's node holds a view
            if tried == 0:
                ev['empty_buckets'] += 1
            assert cnt < st['node_score'].shape[1], 'the store cannot overflow'
            st['node_score'][b, cnt] = tot[h]
            st['node_len'][b, cnt] = L
            st['node_tokens'][b, cnt, :L] = hist
            st['node_att'][b, cnt] = np.asarray(c['att'])[h]
            nb = 0 if states is None else len(states)
            st['node_bag_n'][b, cnt] = nb
            st['node_bag_state'][b, cnt, :nb] = states if nb else []
            st['node_fin'][b, cnt] = 0
            st['node_uplink'][b, cnt] = new_uplink
            slot_node[cur] = cnt
            cnt += 1
        st['node_count'][b] = cnt
    return dict(st, scores=scores, tot=tot), m, ev


def min_margin(m):
    return min(m.values())


def judge_merge(c, got, want, tol):
    """got: the buffers after the launch (NODE_KEYS, scores, tot).  Integers bit-equal, fp32 values
    within tol, -inf exactly where due, and everything the launch must leave alone (frozen
    utterances, node slots behind the count, tokens behind a node's length, bag states behind its
    size) still what it was in c.  -> list of complaints"""
    bad = []
    before = dict(c['store'], scores=c['scores'], tot=c['tot'])

    def same(name, a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'):
            bad.append('%s differs (got %s want %s)' % (name, a.ravel()[:12], b.ravel()[:12]))

    def close(name, a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        fin = np.isfinite(b)
        if a.shape != b.shape or not np.array_equal(a[~fin], b[~fin], equal_nan=True):
            bad.append('%s: non-finite entries differ (got %s want %s)' % (name, a.ravel()[:12], b.ravel()[:12]))
            return
        err = np.abs(a[fin] - b[fin])
        if err.size and not (err <= tol).all():
            bad.append('%s: max error %.3g > tol %.3g' % (name, float(err.max()), tol))

    beam = c['beam']
    for b in range(c['B']):
        sl = slice(b * beam, (b + 1) * beam)
        if int(c['nsteps'][b]) != c['step'] + 1:
            for k in NODE_KEYS:
                same('%s of frozen utterance %d' % (k, b), got[k][b], np.asarray(before[k])[b].astype(got[k].dtype))
            for k in ('scores', 'tot'):
                same('%s of frozen utterance %d' % (k, b), got[k][sl], np.asarray(before[k], np.float32)[sl])
            continue
        n0, n = int(c['store']['node_count'][b]), int(want['node_count'][b])
        same('node_count[%d]' % b, got['node_count'][b], n)
        for k in ('node_len', 'node_bag_n', 'node_fin', 'node_uplink'):
            same('%s[%d]' % (k, b), got[k][b, :n], want[k][b, :n])
        close('node_score[%d]' % b, got['node_score'][b, :n], want['node_score'][b, :n])
        close('scores[%d]' % b, got['scores'][sl], want['scores'][sl])
        close('tot[%d]' % b, got['tot'][sl], want['tot'][sl])
        for i in range(n):
            ln_, nb = int(want['node_len'][b, i]), int(want['node_bag_n'][b, i])
            same('node_tokens[%d, %d]' % (b, i), got['node_tokens'][b, i, :ln_], want['node_tokens'][b, i, :ln_])
            same('node_bag_state[%d, %d]' % (b, i), got['node_bag_state'][b, i, :nb], want['node_bag_state'][b, i, :nb])
            same('node_att[%d, %d]' % (b, i), got['node_att'][b, i], np.asarray(want['node_att'][b, i], np.float32))
            if i >= n0:
                same('node_tokens[%d, %d] behind the length' % (b, i), got['node_tokens'][b, i, ln_:],
                     c['store']['node_tokens'][b, i, ln_:])
                same('node_bag_state[%d, %d] behind the size' % (b, i), got['node_bag_state'][b, i, nb:],
                     c['store']['node_bag_state'][b, i, nb:])
        for k in NODE_KEYS[1:]:
            same('%s[%d] behind the count' % (k, b), got[k][b, n:], np.asarray(c['store'][k])[b, n:])
        for k in ('node_tokens', 'node_att', 'node_bag_state'):
            same('%s[%d] of older nodes' % (k, b), got[k][b, :n0], np.asarray(c['store'][k])[b, :n0])
    return bad


# ------------------------------------------------------------------ the two extra step outputs

def step_extras_ref(c, out):
    """fin_mask [hyps] and tot_out [hyps] of asr_beam_lm_step_graph_f32 in fp64, from the launch's
    inputs c and the referee's outputs `out` (lm_beam_referee.lm_beam_step_ref): the host's
    finish_mask and new_tot_scores.  Rows of frozen utterances: POISON / NaN (left alone)."""
    import torch
    logits = np.asarray(c['logits'], np.float64)
    hyps, C = logits.shape
    B, beam, step, Cm = c['B'], c['beam'], c['step'], C - 1
    fin_mask = np.full(hyps, POISON, np.int32)
    tot = np.full(hyps, np.nan)
    att = np.asarray(c['att'], np.float64)
    for b in range(B):
        if not out['live'][b]:
            continue
        sl = slice(b * beam, (b + 1) * beam)
        ln = int(c['lens'][b])
        x = logits[sl].copy()
        if c.get('min_eos') is not None:
            fl = np.asarray(c['min_eos'], np.float64)[sl]
            x[:, Cm] = np.where(x[:, Cm] > fl, x[:, Cm], fl)
        total = torch.log_softmax(torch.from_numpy(x), 1).numpy() + np.asarray(c['scores_in'], np.float64)[sl, None]
        if c.get('lm_cost') is not None:
            total = total + (-c['lm_weight'] * np.minimum(1e20, np.asarray(c['lm_cost'], np.float64)[sl])
                             ).astype(np.float32).astype(np.float64)
        if c['coverage_weight'] > 0:
            cur = np.asarray(c['cov_in'], np.float64)[sl] + att[sl]
            total = total + (c['coverage_weight'] * (cur[:, :ln] > c['coverage_tau']).sum(1))[:, None]
        fin_mask[sl] = 0
        if step > 0:
            min_pos = np.float32(c['min_attention_pos'] * ln)
            for k in range(beam):
                row = total[k]
                peak = int(np.argmax(att[b * beam + k, :ln])) if ln else 0
                ok = row[Cm] > row[:Cm].max() and np.float32(peak) > min_pos and row[Cm] / c['len_div'] > -1e10
                fin_mask[b * beam + k] = int(bool(ok))
        kb = out['parent'][sl] - b * beam
        t = total[kb, out['new_input'][sl]]
        ncand = (beam if step > 0 else 1) * Cm
        if beam >= ncand:
            t[(ncand if beam > ncand else 0):] = -INF
        tot[sl] = t
    return fin_mask, tot


# ------------------------------------------------------------------ the host layout

def store_graph(store, b, hash_dec, tlen):
    """utterance b of a node store in the host class's layout {hist_hash: [(score, atts, (set of
    states, fin, None), ests, uplink), ...]}: buckets in insertion order, bucket-local uplinks"""
    import torch
    hmap, local, buckets = {}, [], []
    for i in range(int(store['node_count'][b])):
        ests = torch.from_numpy(np.array(store['node_tokens'][b, i, :store['node_len'][b, i]], np.int64))
        li = hmap.setdefault(hash_dec(ests), [])
        local.append(len(li))
        buckets.append(li)
        up = int(store['node_uplink'][b, i])
        nb = int(store['node_bag_n'][b, i])
        li.append((torch.tensor(float(store['node_score'][b, i])), torch.from_numpy(np.array(store['node_att'][b, i, :tlen])),
                   (set(store['node_bag_state'][b, i, :nb].tolist()), bool(store['node_fin'][b, i]), None),
                   ests, None if up < 0 else up))
    for i, li in enumerate(buckets):
        e = li[local[i]]
        if e[4] is not None:
            li[local[i]] = e[:4] + (local[e[4]],)
    return hmap


def hash_dec_of(span):
    def hash_dec(decoded):
        if span == 0:
            return 0
        tail = decoded[-span:].tolist()
        return hash(tuple([-1] * (span - len(tail)) + tail))
    return hash_dec


def graph_arrays(G):
    """get_graph()'s {'V', 'E'} of one utterance as the golden file keeps them -> (V, V scores, E)"""
    V = np.array([[v[0], -1 if v[1] == '<sos>' else v[1], int(bool(v[4]))] for v in G['V']], np.int64)
    E = np.array([[e[0], e[1], int(e[2] == 'merged')] for e in G['E']], np.int64).reshape(-1, 3)
    return V, np.array([v[2] for v in G['V']], np.float64), E


# ------------------------------------------------------------------ trajectories

class RefGraphSearch(lr.RefSearch):
    """lm_beam_referee's chained step with the merge referee behind it: a free-running B-utterance
    graph search in fp64.  `length_normalization` is lm_beam_referee.LN, as RefSearch's len_div."""

    def __init__(self, span, merge_threshold, *args, **kw):
        self.merge_mut = kw.pop('merge_mut', None)
        super(RefGraphSearch, self).__init__(*args, **kw)
        self.span, self.merge_threshold = span, merge_threshold
        self.store = fresh_store(self.B, (self.Lcap - 1) * self.beam, self.Lcap, self.T)
        self.store['node_score'] = self.store['node_score'].astype(np.float64)
        self.merge_margins, self.events = [], collections.Counter()
        self.fin_mask = self.tot = None

    def merge_case(self, c, out, scores, est_in):
        rows = np.repeat(out['live'], self.beam)
        fin_mask, tot = step_extras_ref(c, out)
        use_lm = self.p['lm_weight'] != 0
        return dict(att=np.asarray(c['att']), lens=self.lens, scores=np.where(rows, scores, -INF),
                    tot=np.where(rows, tot, -INF), est_in=est_in, est_out=self.est,
                    fin_mask=np.where(rows, fin_mask, 0), bags=self.bags if use_lm else None,
                    nsteps=np.where(out['live'], c['step'] + 1, -1), parent=np.where(rows, out['parent'], 0),
                    step=c['step'], B=self.B, beam=self.beam, span=self.span,
                    merge_threshold=self.merge_threshold, length_normalization=lr.LN, store=self.store)

    def step(self, logits, att):
        est_in = self.est
        out, c = super(RefGraphSearch, self).step(logits, att)
        rows = np.repeat(out['live'], self.beam)
        mc = self.merge_case(c, out, self.scores, est_in)
        self.fin_mask, self.tot = mc['fin_mask'], mc['tot']
        if self.beam > 1:
            mo, m, ev = merge_ref(mc, self.merge_mut)
            self.merge_margins.append(m)
            self.events.update(ev)
            self.scores = np.where(rows, mo['scores'], self.scores)
            self.tot = mo['tot']
            self.store = {k: mo[k] for k in NODE_KEYS}
        return out, c


# ------------------------------------------------------------------ crafted single launches

CASE_T, CASE_LENS, CASE_LCAP, CASE_STEP, CASE_THR = 12, [12, 9, 6], 12, 3, 0.5


def att_row(peak, tlen, T=CASE_T, gen=None):
    """an alignment over the own `tlen` frames with 0.7 on `peak`; 0.25 of junk behind them, which a
    launch must not read (two rows with the same peak: min-sum 1; different peaks: about 0.3)"""
    a = np.full(T, 0.25, np.float32)
    body = np.full(tlen, 0.3 / (tlen - 1), np.float32)
    if gen is not None:
        body *= (1 + 0.2 * gen.random(tlen)).astype(np.float32)
        body *= 0.3 / (body.sum() - body[peak % tlen])
    body[peak % tlen] = 0.7
    a[:tlen] = body
    return a


def node(tokens, score, peak, states, uplink=-1, fin=0):
    return dict(tokens=list(tokens), score=score, peak=peak, states=sorted(states), uplink=uplink, fin=fin)


def slot(tokens, score, tot, peak, states, parent=None):
    return dict(tokens=list(tokens), score=score, tot=tot, peak=peak, states=sorted(states), parent=parent)


def build_case(utts, span, lm=True, ln=lr.LN, step=CASE_STEP, thr=CASE_THR, T=CASE_T, lens=None, Ncap=None,
               Lcap=CASE_LCAP, seed=0):
    """utts: per utterance dict(nodes=[node()], slots=[slot()] (beam of them), old=[(history of
    `step` labels, finished)] (beam of them), frozen=bool) -> a merge_ref case with POISON-ed store"""
    gen = np.random.default_rng(seed)
    B, beam = len(utts), len(utts[0]['slots'])
    lens = list(CASE_LENS[:B] if lens is None else lens)
    Ncap = (Lcap - 1) * beam if Ncap is None else Ncap
    hyps = B * beam
    store = fresh_store(B, Ncap, Lcap, T, poison=True)
    c = dict(att=np.zeros((hyps, T), np.float32), lens=np.array(lens, np.int32), scores=np.zeros(hyps, np.float32),
             tot=np.zeros(hyps, np.float32), est_in=np.full((hyps, Lcap), POISON, np.int32),
             est_out=np.full((hyps, Lcap), POISON, np.int32), fin_mask=np.zeros(hyps, np.int32),
             bags=[{} for _ in range(hyps)] if lm else None, nsteps=np.zeros(B, np.int32),
             parent=np.zeros(hyps, np.int32), step=step, B=B, beam=beam, span=span, merge_threshold=thr,
             length_normalization=ln, store=store, T=T, Lcap=Lcap)
    for b, u in enumerate(utts):
        c['nsteps'][b] = step if u.get('frozen') else step + 1
        store['node_count'][b] = len(u['nodes'])
        for i, n in enumerate(u['nodes']):
            k = len(n['tokens'])
            store['node_score'][b, i], store['node_len'][b, i] = n['score'], k
            store['node_tokens'][b, i, :k] = n['tokens']
            store['node_att'][b, i] = att_row(n['peak'], lens[b], T, gen)
            store['node_bag_n'][b, i] = len(n['states']) if lm else 0
            if lm:
                store['node_bag_state'][b, i, :len(n['states'])] = n['states']
            store['node_fin'][b, i], store['node_uplink'][b, i] = n['fin'], n['uplink']
        for k, s in enumerate(u['slots']):
            h = b * beam + k
            c['est_out'][h, :step + 1] = s['tokens']
            c['scores'][h], c['tot'][h] = s['score'], s['tot']
            c['att'][h] = att_row(s['peak'], lens[b], T, gen)
            c['parent'][h] = b * beam + (k if s['parent'] is None else s['parent'])
            if lm:
                c['bags'][h] = {q: 0.0 for q in s['states']}
        for k, (hist, fin) in enumerate(u['old']):
            c['est_in'][b * beam + k, :step] = hist
            c['fin_mask'][b * beam + k] = int(fin)
    return c


def _filters_utt():
    """empty bucket, dead candidate, LM-state mismatch, sum below threshold, old branch wins, a -inf
    slot, a finished mark (span 2, step 3)"""
    nodes = [node([3, 4, 5], 9.0, 2, [2, 3], uplink=3),        # dead: has an uplink
             node([5, 4, 5], 9.0, 2, [1]),                     # other LM states
             node([2, 2, 4, 5], 9.0, 8, [2, 3]),               # another alignment
             node([4, 4, 5], -1.0, 2, [2, 3]),                 # -1 / 3^.6 = -0.52 >= -2.5 / 4^.6 = -1.09: wins
             node([5, 5, 5], -3.0, 2, [2, 3])]                 # same length as the finished history, other labels
    slots = [slot([2, 3, 4, 5], -2.0, -2.5, 2, [2, 3]),
             slot([2, 3, 3, 3], -2.2, -2.7, 5, [4]),           # empty bucket
             slot([2, 3, 4, 2], -INF, -INF, 2, [2]),           # a -inf slot appends nothing
             slot([2, 3, 4, 4], -2.4, -2.9, 2, [2])]           # empty bucket
    old = [([4, 4, 5], True), ([2, 3, 4], False), ([5, 5, 4], True), ([3, 4, 5], False)]
    return dict(nodes=nodes, slots=slots, old=old)


def _alias_utt():
    """the new branch wins and drops a descendant that was appended earlier in this launch (alias
    rule) and one whose turn has not come; two new slots in one bucket, the second against a node
    of this launch; the merging slot's parent has another alignment (the column quirk)"""
    nodes = [node([2, 3], -9.0, 2, [2]),                       # loses against slot 1
             node([5, 3], -9.0, 8, [2])]
    slots = [slot([2, 3, 5, 5], -1.0, -1.5, 4, [3]),           # descendant of node 0, appended first
             slot([4, 4, 2, 3], -1.2, -1.7, 2, [2], parent=3), # merges node 0 away: new branch wins
             slot([5, 5, 2, 3], -1.4, -1.9, 2, [2]),           # same bucket: loses to slot 1's node (-1.7 >= -1.9)
             slot([2, 3, 4, 4], -1.6, -2.1, 8, [2])]           # descendant of node 0, dropped before its turn
    old = [([2, 3, 5], False), ([4, 4, 2], False), ([5, 5, 2], False), ([2, 3, 4], False)]
    return dict(nodes=nodes, slots=slots, old=old)


def _frozen_utt():
    u = _filters_utt()
    u['frozen'] = True
    return u


def _tie_utt(ln_zero_score=-2.5):
    nodes = [node([4, 4, 5], ln_zero_score, 2, [2, 3]),
             node([2, 3, 4, 5], -3.3, 2, [2, 3])]              # slot 0's own sequence: a key of any span matches
    slots = [slot([2, 3, 4, 5], -2.0, ln_zero_score, 2, [2, 3]), slot([2, 3, 3, 3], -2.2, -2.7, 5, [4]),
             slot([2, 3, 4, 2], -2.3, -2.8, 2, [2]), slot([2, 3, 4, 4], -2.4, -2.9, 2, [2])]
    old = [([4, 4, 5], False), ([2, 3, 4], False), ([5, 5, 4], False), ([3, 4, 5], False)]
    return dict(nodes=nodes, slots=slots, old=old)


def big_case(seed=1):
    """beam 32, T 130 (more than a wave, no multiple of 64), 300 older nodes (more than one pass of
    256 threads) over a two-label alphabet, so that buckets are full"""
    gen = np.random.default_rng(seed)
    beam, T, step, lens = 32, 130, 2, [130, 77]
    utts = []
    for b in range(2):
        nodes = [node(gen.integers(2, 4, int(gen.integers(1, 3))).tolist(), float(gen.normal(-4, 2)),
                      int(gen.integers(0, 3)) * 31, [int(gen.integers(1, 3))],
                      uplink=int(gen.integers(0, 300)) if gen.random() < 0.3 else -1) for _ in range(300)]
        slots = [slot(gen.integers(2, 4, 3).tolist(), float(gen.normal(-3, 1)), float(gen.normal(-4, 2)),
                      int(gen.integers(0, 3)) * 31, [int(gen.integers(1, 3))]) for _ in range(beam)]
        for k in (5, 17):
            slots[k]['score'] = slots[k]['tot'] = -INF
        old = [(gen.integers(2, 4, 2).tolist(), bool(gen.random() < 0.3)) for _ in range(beam)]
        utts.append(dict(nodes=nodes, slots=slots, old=old))
    return build_case(utts, 1, step=step, T=T, lens=lens, Ncap=352, Lcap=8, seed=seed)


def merge_cases():
    """name -> case; B 3, beam 4, T 12 except `big`"""
    three = lambda: [_filters_utt(), _alias_utt(), _frozen_utt()]  # noqa: E731
    live = lambda: [_filters_utt(), _alias_utt(), _tie_utt(-2.6)]  # noqa: E731
    return {
        'span2': build_case(three(), 2),
        'span0': build_case(live(), 0),                          # every node in one bucket
        'span_longer_than_history': build_case(live(), 9),
        'no_lm_term': build_case(live(), 2, lm=False),
        'tie': build_case([_tie_utt(), _alias_utt(), _tie_utt()], 2, ln=0.0),   # -2.5 >= -2.5: the old branch wins
        'big': big_case(),
    }


def merge_graphs_of(store, b, hash_dec, tlen):
    """get_graph() of utterance b of a node store: the host class's own code on the host layout"""
    from att_speech.modules.beam_search import merge_graphs
    return merge_graphs([store_graph(store, b, hash_dec, tlen)])[0]


def traj_inputs(B, beam, C, steps, seed, lens, T):
    """lm_beam_referee.traj_inputs for T frames, with peaks that depend on the parity of the slot
    only: slots of one parity have near-equal alignments (min-sum about 0.65), the others about 0.35"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    logits = 4 * torch.randn(steps, B * beam, C, generator=gen)
    for b in range(B):
        logits[:, b * beam:(b + 1) * beam, -1] += (0.0, 2.0, 5.0)[b % 3]
    att = np.stack([lr.peaked_att(gen, B * beam, T, lens, beam) for _ in range(steps)])
    for s in range(steps):
        for h in range(B * beam):
            ln = lens[h // beam]
            a = att[s, h, :ln]
            k = int(np.argmax(a))
            tgt = min(ln - 1, (s * ln) // 4 + (h % 2))
            a[k], a[tgt] = a[tgt], a[k]
    return logits.numpy(), att
