"""The fp64 referees of tests/recurrence_referee.py and their acceptance rule, proved on the CPU
before they judge a kernel (tests/test_recurrence_referee_gpu.py):

* with the bf16 rounding switched off, the free-running references are torch double autograd
  (a cell loop of plain torch ops, and nn.LSTM / nn.GRU on a packed batch) to 1e-10;
* a stand-in kernel, the same recurrences free-running in fp32 with a permuted summation order,
  the kernels' exp / reciprocal forms of sigma and tanh and bf16 rounding where the kernels
  round, passes the teacher-forced rule with zero violations at every case of the GPU matrix
  that is cheap enough for the CPU: the radius is not too tight;
* seeded mutants of the stand-in, one wrong term each, violate it wherever the term is live:
  the rule discriminates;
* the radius stays under a quarter bf16 ulp on >= 95 % of the checked elements and the
  sub-normal branch takes <= 0.1 % of them: the radius cannot hide a failure.

Measured on the CPU.  Violating elements summed over the cases where the mutant is live (40 cases
of the matrix are small enough for the mutants), smallest count of any single live case last:

    mutant               pass  live cases  violations  min per case
    d_o_without_1-o      bwd   26            8070666   1022
    c_t_for_c_t-1        bwd   26            8126690   1022
    c_t-1_not_zeroed     bwd   26             701649    128
    dc_carry_not_reset   bwd   29            7314971   3968
    reverse_from_T-1     fwd   29            1098261   6030
    other_dy_plane       bwd   23           26561297   1784
    i_f_swapped          fwd   26           16666296   2036
    r_z_swapped (GRU)    fwd   17           11484953   1020
    h_from_t-2           fwd   40           60871618    403
    dgates_from_t-2      bwd   40           43354658    278
    dhn_for_dn (GRU)     bwd   17            4929920    511
    h_prev-n_sign (GRU)  bwd   17            5641917    511

The unmutated stand-in: zero violations at all 47 cases small enough for the CPU, and on
synthetic saved tensors.

The caps (test_radius_is_below_a_quarter_ulp_on_95_percent).  The worst-case dot-product bound
(K + 8) 2^-24 sum|a_k b_k| grows like K while the magnitude of the sum grows like sqrt(K), so at
the base draw (gx ~ 1.5 N, W_hh ~ N/sqrt(H)) the share of elements with a radius under a quarter
ulp falls from 98.9 % (LSTM, H = 64) to 69.2 % (H = 768; GRU 98.5 % -> 86.7 % at H = 320), and
3.8 % of the tanh records saturate to exactly +-1 in bf16, whose gradients are exact zeros: the
sub-normal branch takes 0.28 % (LSTM) / 0.92 % (GRU).  The inputs of the cap test were therefore
changed, not the caps: the quiet draw (recurrence_referee.quiet: gx ~ 0.8 N, W_hh ~ N/(2H), so
that sum|a_k b_k| does not grow with H) and T = 320 (d_f, and the GRU's hn and dr, of an
utterance's first frame are exactly zero whatever the inputs).  Measured there:

    LSTM H =  64 128 256 320 384 512 768      radius < ulp/4 on  99.62 99.28 98.63 98.29 97.95 97.28 95.94 %
    GRU  H =  64 128 256 320                                     99.26 98.46 96.76 95.45 %
    sub-normal branch: 0.031 % (LSTM), 0.070 % (GRU) at every H

The quiet draw is part of the GPU matrix beside the base and the saturated one, which load the
recurrent product with the wider radius.
"""
import pytest
import torch
from torch import nn

import recurrence_referee as rr
from recurrence_referee import F64

CHEAP = [c for c in rr.CASES if c['T'] * c['B'] * c['H'] ** 2 <= 3e9 and not c['fused']]


def _s(x):
    return 1 / (1 + torch.exp(-x))


def _t(x):
    return 2 / (1 + torch.exp(-2 * x)) - 1


def _bf(x):
    return x.to(torch.bfloat16).float()


def _act(T, lens, frames):
    act = rr.act_mask(T, lens)
    return torch.stack([act[frames[0]], act[frames[1]]])[:, :, None]


def _get(x, frames, dirdim, T, act=None):
    out = []
    for d, t in enumerate(frames):
        if 0 <= t < T:
            v = x[t].select(dirdim, d).float()
            if act is not None:
                v = v * act[t].view(-1, *([1] * (v.dim() - 1)))
        else:
            v = torch.zeros_like(x[0].select(dirdim, d), dtype=torch.float32)
        out.append(v)
    return torch.stack(out)


# ---------------------------------------------------------------- the stand-in kernels (fp32)

def standin_lstm_fwd(gx, whh, lens, mut=None, seed=0):
    T, B, _, H4 = gx.shape
    H = H4 // 4
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(seed))
    wt = whh.float().transpose(1, 2)[:, perm].contiguous()
    y = torch.zeros(T, B, 2, H)
    gates = torch.full((T, 2, B, H, 4), 0.5).to(torch.bfloat16)        # junk on padding frames
    csave = torch.full((T, 2, B, H), 0.7)
    h, c, h2 = torch.zeros(2, B, H), torch.zeros(2, B, H), torch.zeros(2, B, H)
    for s in range(T):
        cur = (s, T - 1 - s)
        a = _act(T, lens, cur)
        hop = _bf(h2 if mut == 'h_from_t-2' else h)
        pre = (_get(gx, cur, 1, T) + torch.bmm(hop[:, :, perm], wt)).view(2, B, 4, H)
        gi, gf, gg, go = _s(pre[:, :, 0]), _s(pre[:, :, 1]), _t(pre[:, :, 2]), _s(pre[:, :, 3])
        cn = gf * c + gi * gg
        hn = go * _t(cn)
        rec = torch.stack([gf, gi, gg, go] if mut == 'i_f_swapped' else [gi, gf, gg, go], -1).to(torch.bfloat16)
        for d, t in enumerate(cur):
            m = a[d, :, 0]
            gates[t, d][m] = rec[d][m]
            csave[t, d][m] = cn[d][m]
            y[t, :, d][m] = hn[d][m]
        keep = a.clone()
        if mut == 'reverse_from_T-1':
            keep[1] = True
        h2 = h
        h, c = hn * keep, cn * keep
    ybf = torch.zeros(2, T + 2, B, H, dtype=torch.bfloat16)
    ybf[:, 1:T + 1] = y.to(torch.bfloat16).permute(2, 0, 1, 3)
    return y, ybf, gates, csave


def standin_lstm_bwd(dy, shared, whhT, lens, gates, csave, mut=None, seed=0):
    T, B, H = dy.shape[0], dy.shape[1], dy.shape[-1]
    perm = torch.randperm(4 * H, generator=torch.Generator().manual_seed(seed + 1))
    m = whhT.float().transpose(1, 2)[:, perm].contiguous()
    act = rr.act_mask(T, lens)
    dg = torch.zeros(T, B, 2, 4 * H, dtype=torch.bfloat16)
    op, op2, carry = torch.zeros(2, B, 4 * H), torch.zeros(2, B, 4 * H), torch.zeros(2, B, H)
    for s in range(T):
        cur, prv = (T - 1 - s, s), (T - 2 - s, s + 1)
        a = _act(T, lens, cur)
        if shared:
            dyt = torch.stack([dy[cur[0]], dy[cur[1]]])
        elif mut == 'other_dy_plane':
            dyt = torch.stack([dy[cur[0], :, 1], dy[cur[1], :, 0]])
        else:
            dyt = torch.stack([dy[cur[0], :, 0], dy[cur[1], :, 1]])
        src = op2 if mut == 'dgates_from_t-2' else op
        dh = dyt + torch.bmm(src[:, :, perm], m)
        gi, gf, gg, go = _get(gates, cur, 0, T).unbind(-1)
        cs = _get(csave, cur, 0, T)
        if mut == 'c_t_for_c_t-1':
            cp = cs
        elif mut == 'c_t-1_not_zeroed':
            cp = _get(csave, tuple(p % T for p in prv), 0, T)
        else:
            cp = _get(csave, prv, 0, T, act)
        tc = _t(cs)
        dc = dh * go * (1 - tc * tc) + carry
        d_o = dh * tc * go if mut == 'd_o_without_1-o' else dh * tc * go * (1 - go)
        d = torch.stack([dc * gg * gi * (1 - gi), dc * cp * gf * (1 - gf), dc * gi * (1 - gg * gg), d_o], 2)
        d = _bf(d * a[..., None]).view(2, B, 4 * H)
        for k, t in enumerate(cur):
            dg[t, :, k] = d[k].to(torch.bfloat16)
        carry = dc * gf
        if mut != 'dc_carry_not_reset':
            carry = carry * a
        op2, op = op, d
    return dg


def standin_gru_fwd(gx, whh, lens, mut=None, seed=0):
    T, B, _, H3 = gx.shape
    H = H3 // 3
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(seed))
    wt = whh.float().transpose(1, 2)[:, perm].contiguous()
    y = torch.zeros(T, B, 2, H)
    gates = torch.full((T, 2, B, H, 4), 0.5).to(torch.bfloat16)
    h, h2 = torch.zeros(2, B, H), torch.zeros(2, B, H)
    for s in range(T):
        cur = (s, T - 1 - s)
        a = _act(T, lens, cur)
        hop = _bf(h2 if mut == 'h_from_t-2' else h)
        g = _get(gx, cur, 1, T).view(2, B, 3, H)
        rec = torch.bmm(hop[:, :, perm], wt).view(2, B, 3, H)
        r, z, hn = _s(g[:, :, 0] + rec[:, :, 0]), _s(g[:, :, 1] + rec[:, :, 1]), rec[:, :, 2]
        n = _t(g[:, :, 2] + r * hn)
        hnew = (1 - z) * n + z * h
        rc = torch.stack([z, r, n, hn] if mut == 'r_z_swapped' else [r, z, n, hn], -1).to(torch.bfloat16)
        for d, t in enumerate(cur):
            m = a[d, :, 0]
            gates[t, d][m] = rc[d][m]
            y[t, :, d][m] = hnew[d][m]
        keep = a.clone()
        if mut == 'reverse_from_T-1':
            keep[1] = True
        h2 = h
        h = hnew * keep
    ybf = torch.zeros(2, T + 2, B, H, dtype=torch.bfloat16)
    ybf[:, 1:T + 1] = y.to(torch.bfloat16).permute(2, 0, 1, 3)
    return y, ybf, gates


def standin_gru_bwd(dy, shared, whhT, lens, gates, y, mut=None, seed=0):
    T, B, H = dy.shape[0], dy.shape[1], dy.shape[-1]
    perm = torch.randperm(3 * H, generator=torch.Generator().manual_seed(seed + 1))
    m = whhT.float().transpose(1, 2)[:, perm].contiguous()
    act = rr.act_mask(T, lens)
    dgx = torch.zeros(T, B, 2, 3 * H, dtype=torch.bfloat16)
    dhn = torch.zeros(T, B, 2, H, dtype=torch.bfloat16)
    op, op2, carry = torch.zeros(2, B, 3 * H), torch.zeros(2, B, 3 * H), torch.zeros(2, B, H)
    for s in range(T):
        cur, prv = (T - 1 - s, s), (T - 2 - s, s + 1)
        a = _act(T, lens, cur)
        if shared:
            dyt = torch.stack([dy[cur[0]], dy[cur[1]]])
        elif mut == 'other_dy_plane':
            dyt = torch.stack([dy[cur[0], :, 1], dy[cur[1], :, 0]])
        else:
            dyt = torch.stack([dy[cur[0], :, 0], dy[cur[1], :, 1]])
        src = op2 if mut == 'dgates_from_t-2' else op
        dh = (dyt + carry) + torch.bmm(src[:, :, perm], m)
        r, z, n, hn = _get(gates, cur, 0, T).unbind(-1)
        hp = _get(y, prv, 1, T, act)
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * ((n - hp) if mut == 'h_prev-n_sign' else (hp - n)) * z * (1 - z)
        d = torch.stack([dn * hn * r * (1 - r), dz, dn * r if mut == 'dhn_for_dn' else dn, dn * r], 2)
        d = _bf(d * a[..., None])
        for k, t in enumerate(cur):
            dgx[t, :, k] = d[k, :, :3].reshape(B, 3 * H).to(torch.bfloat16)
            dhn[t, :, k] = d[k, :, 3].to(torch.bfloat16)
        carry = dh * z
        if mut != 'dc_carry_not_reset':
            carry = carry * a
        op2, op = op, torch.cat([d[:, :, 0], d[:, :, 1], d[:, :, 3]], -1)
    return dgx, dhn


# ---------------------------------------------------------------- refereeing a stand-in run

def _inputs(c):
    seed = c['T'] * 1009 + c['B'] * 31 + c['H']
    inp = rr.make_inputs(c['rnn'], c['T'], c['B'], c['H'], c['kind'], seed, c['gx_scale'], c['dy_shared'], c['w_scale'])
    if c['gx_bf16']:
        inp['gx'] = inp['gx'].to(torch.bfloat16)
    return inp


_FWD_CACHE = {}


def referee_standin(c, mut_f=None, mut_b=None, passes=('fwd', 'bwd')):
    """-> (forward verdict, backward verdict) of the stand-in with the given mutation"""
    inp = _inputs(c)
    lens, H = inp['lens'], c['H']
    key = (rr.case_id(c), mut_f)
    if key not in _FWD_CACHE:
        _FWD_CACHE.clear()
        _FWD_CACHE[key] = (standin_lstm_fwd if c['rnn'] == 'lstm' else standin_gru_fwd)(
            inp['gx'], inp['whh'], lens, mut_f)
    fw = _FWD_CACHE[key]
    vf, vb = rr.Verdict(), rr.Verdict()
    if c['rnn'] == 'lstm':
        y, ybf, gates, csave = fw
        if 'fwd' in passes:
            want = rr.lstm_forward(inp['gx'], inp['whh'], lens, forced=(ybf, csave))
            rr.judge_lstm_forward(vf, want, y, ybf, gates, csave, lens)
        if 'bwd' in passes:
            dg = standin_lstm_bwd(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, csave, mut_b)
            want = rr.lstm_backward(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, csave, forced=dg)
            rr.judge_backward(vb, want, {'dgates': dg}, lens, H)
    else:
        y, ybf, gates = fw
        if 'fwd' in passes:
            want = rr.gru_forward(inp['gx'], inp['whh'], lens, forced=(ybf, y))
            rr.judge_gru_forward(vf, want, y, ybf, gates, lens)
        if 'bwd' in passes:
            dgx, dhn = standin_gru_bwd(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, y, mut_b)
            want = rr.gru_backward(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, y, forced=(dgx, dhn))
            rr.judge_backward(vb, want, {'dgx': dgx, 'dhn': dhn}, lens, H)
    return vf, vb


@pytest.mark.parametrize('c', CHEAP, ids=rr.case_id)
def test_fp32_standin_passes_with_zero_violations(c):
    vf, vb = referee_standin(c)
    assert vf.checked and vb.checked
    assert vf.count == 0, 'forward: ' + vf.report()
    assert vb.count == 0, 'backward: ' + vb.report()


def test_synthetic_saved_tensors_pass_for_the_standin():
    """the second backward run of the GPU test: saved tensors the forward would rarely produce"""
    for c in CHEAP[::5]:
        inp = _inputs(c)
        lens, H = inp['lens'], c['H']
        gates, other = rr.synthetic_saved(c['rnn'], c['T'], c['B'], H, lens, 5)
        v = rr.Verdict()
        if c['rnn'] == 'lstm':
            dg = standin_lstm_bwd(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, other)
            want = rr.lstm_backward(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, other, forced=dg)
            rr.judge_backward(v, want, {'dgates': dg}, lens, H)
        else:
            dgx, dhn = standin_gru_bwd(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, other)
            want = rr.gru_backward(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, other, forced=(dgx, dhn))
            rr.judge_backward(v, want, {'dgx': dgx, 'dhn': dhn}, lens, H)
        assert v.count == 0, rr.case_id(c) + ': ' + v.report()


# ---------------------------------------------------------------- mutants

def _ragged(c):             # some utterance has a padding frame
    return c['kind'] != 'full' and c['T'] > 1 and c['B'] > 1


# name -> (rnn or None for both, pass, where the mutated term is live)
MUTANTS = {
    'd_o_without_1-o': ('lstm', 'bwd', lambda c: True),
    'c_t_for_c_t-1': ('lstm', 'bwd', lambda c: True),
    'c_t-1_not_zeroed': ('lstm', 'bwd', lambda c: True),
    'dc_carry_not_reset': (None, 'bwd', _ragged),
    'reverse_from_T-1': (None, 'fwd', _ragged),
    'other_dy_plane': (None, 'bwd', lambda c: not c['dy_shared']),
    'i_f_swapped': ('lstm', 'fwd', lambda c: True),
    'r_z_swapped': ('gru', 'fwd', lambda c: True),
    'h_from_t-2': (None, 'fwd', lambda c: c['T'] >= 2 and (c['kind'] != 'one_long' or c['T'] >= 2)),
    'dgates_from_t-2': (None, 'bwd', lambda c: c['T'] >= 2),
    'dhn_for_dn': ('gru', 'bwd', lambda c: True),
    'h_prev-n_sign': ('gru', 'bwd', lambda c: True),
}

MUTANT_CASES = [c for c in CHEAP if c['T'] * c['B'] * c['H'] ** 2 <= 4e8]


def mutant_counts(name):
    rnn, which, live = MUTANTS[name]
    rows = []
    for c in MUTANT_CASES:
        if (rnn is not None and c['rnn'] != rnn) or not live(c):
            continue
        vf, vb = referee_standin(c, mut_f=name if which == 'fwd' else None,
                                 mut_b=name if which == 'bwd' else None, passes=(which,))
        rows.append((rr.case_id(c), (vf if which == 'fwd' else vb).count))
    return rows


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_mutant_is_caught_wherever_it_is_live(name):
    rows = mutant_counts(name)
    assert len(rows) >= 4, rows
    print('%-20s %s  live cases %3d  violations %9d (min %d)' % (
        name, MUTANTS[name][1], len(rows), sum(n for _, n in rows), min(n for _, n in rows)))
    missed = [cid for cid, n in rows if n == 0]
    assert not missed, missed


# ---------------------------------------------------------------- the radius cannot hide a failure

# d_f of an utterance's first frame is exactly zero (c_{t-1} = 0), a quarter of the gate gradients
# of that frame: utterances must be long for the sub-normal branch to stay under 0.1 %
CAP_CASES = [rr.case(rnn, 320, 3, H, 'stair', gx_bf16=H % 128 == 0, dy_shared=H % 3 == 0,
                     gx_scale=rr.quiet(H)[0], w_scale=rr.quiet(H)[1])
             for rnn, hs in (('lstm', (64, 128, 256, 320, 384, 512, 768)), ('gru', (64, 128, 256, 320))) for H in hs]


@pytest.mark.parametrize('rnn,H', [('lstm', h) for h in (64, 128, 256, 320, 384, 512, 768)] +
                         [('gru', h) for h in (64, 128, 256, 320)])
def test_radius_is_below_a_quarter_ulp_on_95_percent(rnn, H):
    """At gx ~ 1.5 N(0,1), W_hh ~ N(0,1)/sqrt(H), dy ~ N(0,1) (the mid-length cases of the matrix;
    the saturated draw with its exactly zero gradients is judged by the rule but not counted
    here), from the referee alone: its own free-running bf16 evaluation is the teacher."""
    tight = tiny = checked = 0
    for c in CAP_CASES:
        if c['rnn'] != rnn or c['H'] != H:
            continue
        inp = _inputs(c)
        lens = inp['lens']
        act = rr.act_mask(c['T'], lens)
        v = rr.Verdict()
        if rnn == 'lstm':
            w = rr.lstm_forward(inp['gx'], inp['whh'], lens)
            rr.judge_lstm_forward(v, w, w['y'].float(), torch.zeros(2, c['T'] + 2, c['B'], H, dtype=torch.bfloat16),
                                  w['gates'], w['csave'], lens)
            gates = rr.bf16_round(w['gates'])
            b = rr.lstm_backward(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, w['csave'].float())
            rr.judge_backward(v, b, {'dgates': b['dgates']}, lens, H)
        else:
            w = rr.gru_forward(inp['gx'], inp['whh'], lens)
            rr.judge_gru_forward(v, w, w['y'].float(), torch.zeros(2, c['T'] + 2, c['B'], H, dtype=torch.bfloat16),
                                 w['gates'], lens)
            gates = rr.bf16_round(w['gates'])
            b = rr.gru_backward(inp['dy'], c['dy_shared'], inp['whhT'], lens, gates, w['y'].float())
            rr.judge_backward(v, b, {'dgx': b['dgx'], 'dhn': b['dhn']}, lens, H)
        tight, tiny, checked = tight + v.tight, tiny + v.tiny, checked + v.checked
    assert checked
    print('%s H=%d: radius < ulp/4 on %.2f %%, sub-normal branch %.4f %% of %d elements' % (
        rnn, H, 100.0 * tight / checked, 100.0 * tiny / checked, checked))
    assert tight >= 0.95 * checked, (tight, checked)
    assert tiny <= 0.001 * checked, (tiny, checked)


# ---------------------------------------------------------------- the referee is autograd

def _close(a, b, what):
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= 1e-10 * scale, (what, err, scale)


def _cell_loop(rnn, gx, whh, lens):
    """double-precision cell loop of plain torch ops -> y [T,B,2,H] (and the GRU's hn [T,B,2,H])"""
    T, B = gx.shape[:2]
    H = whh.shape[-1]
    act = rr.act_mask(T, lens)
    ys, hns = [[None] * T, [None] * T], [[None] * T, [None] * T]
    for d in range(2):
        h = torch.zeros(B, H, dtype=F64)
        c = torch.zeros(B, H, dtype=F64)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = act[t][:, None]
            rec = h @ whh[d].t()
            if rnn == 'lstm':
                i, f, g, o = (gx[t, :, d] + rec).chunk(4, -1)
                cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                hn = torch.sigmoid(o) * torch.tanh(cn)
                c = torch.where(a, cn, torch.zeros_like(cn))
            else:
                gr, gz, gn = gx[t, :, d].chunk(3, -1)
                ar, az, hh = rec.chunk(3, -1)
                hns[d][t] = torch.zeros(B, H, dtype=F64, requires_grad=True)      # d/d(hn) lands here
                hh = hh + hns[d][t]
                r, z = torch.sigmoid(gr + ar), torch.sigmoid(gz + az)
                n = torch.tanh(gn + r * hh)
                hn = (1 - z) * n + z * h
            h = torch.where(a, hn, torch.zeros_like(hn))
            ys[d][t] = h
    return torch.stack([torch.stack(ys[0]), torch.stack(ys[1])], 2), hns


@pytest.mark.parametrize('rnn', ['lstm', 'gru'])
@pytest.mark.parametrize('kind,T,B,H,shared', [
    ('ragged', 9, 7, 16, False), ('ragged', 12, 5, 24, True), ('full', 5, 3, 16, False),
    ('one_long', 6, 4, 16, True), ('stair', 30, 34, 8, False), ('full', 1, 1, 16, False)])
def test_free_running_referee_is_double_autograd(rnn, kind, T, B, H, shared):
    G = 4 if rnn == 'lstm' else 3
    inp = rr.make_inputs(rnn, T, B, H, kind, 11 + T, dy_shared=shared)
    lens = inp['lens']
    whh = inp['whh'].to(F64) + 1e-3 * torch.randn(2, G * H, H, dtype=F64,
                                                  generator=torch.Generator().manual_seed(1))   # not bf16 values
    gx = inp['gx'].to(F64).requires_grad_()
    dy = inp['dy'].to(F64)
    act = rr.act_mask(T, lens)
    y, hns = _cell_loop(rnn, gx, whh, lens)
    dyf = (torch.stack([dy, dy], 2) if shared else dy) * act[:, :, None, None]
    (y * dyf).sum().backward()
    if rnn == 'lstm':
        w = rr.lstm_forward(gx.detach(), whh, lens, round_h=False)
        b = rr.lstm_backward(dy, shared, whh.transpose(1, 2), lens, w['gates'], w['csave'], round_d=False)
        _close(b['dgates'], gx.grad, 'dgates')
    else:
        w = rr.gru_forward(gx.detach(), whh, lens, round_h=False)
        b = rr.gru_backward(dy, shared, whh.transpose(1, 2), lens, w['gates'], w['y'], round_d=False)
        _close(b['dgx'], gx.grad, 'dgx')
        dhn = torch.zeros(T, B, 2, H, dtype=F64)
        for d in range(2):
            for t in range(T):
                dhn[t, :, d] = hns[d][t].grad * act[t][:, None]
        _close(b['dhn'], dhn, 'dhn')
    _close(w['y'], y.detach(), 'y')
    assert not gx.grad[~act].any() and not w['y'][~act].any()

    # and torch's own cell on a packed batch, W_ih = I so that gx is the input
    mod = (nn.LSTM if rnn == 'lstm' else nn.GRU)(2 * G * H, H, bidirectional=True, bias=False).double()
    eye = torch.eye(G * H, dtype=F64)
    zero = torch.zeros(G * H, G * H, dtype=F64)
    with torch.no_grad():
        mod.weight_ih_l0.copy_(torch.cat([eye, zero], 1))
        mod.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], 1))
        mod.weight_hh_l0.copy_(whh[0])
        mod.weight_hh_l0_reverse.copy_(whh[1])
    x = gx.detach().clone()
    x[~act] = 0                                     # the packed batch never sees the padding
    x = x.view(T, B, 2 * G * H).requires_grad_()
    out, _ = nn.utils.rnn.pad_packed_sequence(mod(nn.utils.rnn.pack_padded_sequence(x, lens))[0], total_length=T)
    (out.view(T, B, 2, H) * dyf).sum().backward()
    _close(w['y'], out.detach().view(T, B, 2, H), 'y vs nn')
    _close(b['dgates' if rnn == 'lstm' else 'dgx'], x.grad.view(T, B, 2, G * H), 'dgx vs nn')


def test_the_rule_itself():
    """round_down / round_up bracket every double by neighbouring bf16 numbers, and the rule
    accepts exactly the bf16 numbers inside the widened interval"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, dtype=F64, generator=g) * torch.exp(8 * torch.randn(4096, dtype=F64, generator=g))
    lo, hi = rr.bf16_round_down(x), rr.bf16_round_up(x)
    for v in (lo, hi):
        assert torch.equal(v.to(torch.bfloat16).to(F64), v)           # representable
    assert bool((lo <= x).all()) and bool((x <= hi).all())
    assert bool(((hi - lo) <= rr.bf16_ulp(x)).all())
    assert torch.equal(rr.bf16_round(x), x.float().to(torch.bfloat16).to(F64)) or \
        int((rr.bf16_round(x) != x.float().to(torch.bfloat16).to(F64)).sum()) <= 2   # double rounding via fp32
    zero = torch.zeros_like(x)
    assert not rr.violations(lo, x, zero, True).any() and not rr.violations(hi, x, zero, True).any()
    assert rr.violations(lo - rr.bf16_ulp(lo), x, zero, True).all()
    assert rr.violations(hi + rr.bf16_ulp(hi), x, zero, True).all()
    assert rr.violations(torch.full((1,), float('nan')), torch.ones(1, dtype=F64), torch.ones(1, dtype=F64), True).all()
    assert not rr.violations(torch.zeros(1), torch.full((1,), 1e-40, dtype=F64), torch.zeros(1, dtype=F64), False).any()
    assert rr.violations(torch.full((1,), 1e-30), torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64), True).all()
