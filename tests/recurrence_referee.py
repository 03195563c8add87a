"""fp64 referees of the BiLSTM / BiGRU recurrences (include/asr_amd.h, asr_lstm_bidir_* and
asr_gru_bidir_*), one time step at a time.

The recurrences feed back only values they also write out (y_bf16, csave, dgates, dgx, dhn, y),
so a reference can take the kernel's own output of the neighbouring frame as the recurrent
operand (`forced=`, teacher forcing) and judge every step on its own: the drift of a free-
running comparison, where one flipped bf16 rounding of h changes everything after it, is gone,
and a bound of about one bf16 ulp per element becomes possible.  Without `forced` the same
functions run free (their own state fed back), which is how they are proved against torch
autograd in tests/test_recurrence_referee.py.

Every function returns, beside the expected values, a per-element error radius derived from
the arithmetic the header documents (bf16 operands, fp32 accumulation / gates / state):

* a K-term fp32 dot product plus addends: (K + 8) * 2^-24 * (sum |a_k b_k| + sum |addends|);
* through sigma / tanh by Taylor's theorem: |f'(x)| d + max|f''|/2 d^2 (max|sigma''| < 0.1,
  max|tanh''| < 0.77), where d also holds 2^-22 |x| for the rounding of the scaled exp2
  argument; tanh is formed as 2 / (1 + 2^(-2x log2 e)) - 1, whose absolute error does not shrink
  with |tanh| (2^-23 from exp2, 2^-23 from the sum at 2, 2^-24 from rcp at 1/2, doubled: 2^-22);
* products and sums to first order plus the product of the radii; a sum that can cancel gets
  2^-22 of the magnitudes of its terms;
* 2^-20 |want| for the hardware exp2 / rcp and the pointwise fp32 roundings;
* the radius of a carried value (dc, the GRU's dh * z) travels with the value.

Layouts are the header's: gx [T,B,2,G*H], y [T,B,2,H], y_bf16 [2,T+2,B,H], gates [T,2,B,H,4],
csave [T,2,B,H], dy [T,B,2,H] or [T,B,H], dgates / dgx [T,B,2,G*H], dhn [T,B,2,H]."""
import torch

U = 2.0 ** -24
F64 = torch.float64


def act_mask(T, lens):
    """[T,B] bool: utterance b is active at frame t iff t < lens[b]"""
    return torch.arange(T)[:, None] < torch.as_tensor(lens).long()[None, :]


# ------------------------------------------------------------------ bf16 on doubles

def bf16_ulp(x):
    """spacing of bf16 numbers at |x| (8 significant bits; the smallest normal binade below)"""
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.ones_like(x), e.clamp(min=-125) - 8)


def bf16_round_down(x):
    u = bf16_ulp(x)
    return torch.floor(x / u) * u


def bf16_round_up(x):
    u = bf16_ulp(x)
    return torch.ceil(x / u) * u


def bf16_round(x):
    """round to nearest even, on doubles (no double rounding through fp32)"""
    u = bf16_ulp(x)
    return torch.round(x / u) * u


TINY = 2.0 ** -126          # below: bf16 subnormals, flushed or not


def violations(got, want, delta, bf16):
    """The acceptance rule.  bf16 output: bf16_round_down(want - d) <= got <= bf16_round_up(want + d);
    fp32 output: |got - want| <= d; |want| below the bf16 normal range: |got| <= 2^-120 + d.
    Returns the bool tensor of violating elements (NaN violates)."""
    got = got.to(F64)
    if bf16:
        ok = (got >= bf16_round_down(want - delta)) & (got <= bf16_round_up(want + delta))
    else:
        ok = (got - want).abs() <= delta
    tiny = want.abs() < TINY
    ok = torch.where(tiny, got.abs() <= 2.0 ** -120 + delta, ok)
    return ~ok


def ulp_error(got, want):
    """|got - want| in bf16 ulps of want"""
    return (got.to(F64) - want).abs() / bf16_ulp(want)


# ------------------------------------------------------------------ pointwise maps with radii

def _sig(x, dx):
    v = torch.sigmoid(x)
    d = dx + 2.0 ** -22 * x.abs()
    return v, v * (1 - v) * d + 0.05 * d * d + 2.0 ** -20 * v


def _tanh(x, dx):
    v = torch.tanh(x)
    d = dx + 2.0 ** -22 * x.abs()
    return v, (1 - v * v) * d + 0.4 * d * d + 2.0 ** -22 + 2.0 ** -20 * v.abs()


def _dot(a, w, wabs32):
    """a [2,B,K] . w [2,K,N] in fp64, and sum |a_k w_k| (fp32 is plenty for a bound: 1e-5 added)"""
    return torch.bmm(a, w), torch.bmm(a.abs().float(), wabs32).double() * (1 + 1e-5)


def _pick(x, frames, dirdim, act=None):
    """slab [2, B, ...]: x[frames[d]] of direction d for d = 0, 1 (x is [T, ...] with the direction
    at `dirdim` of x[t]); zero where the frame is outside [0, T) or, with `act`, inactive"""
    T = x.shape[0]
    out = []
    for d, t in enumerate(frames):
        if 0 <= t < T:
            v = x[t].select(dirdim, d).to(F64)
            if act is not None:
                a = act[t]
                v = torch.where(a.view(-1, *([1] * (v.dim() - 1))), v, torch.zeros_like(v))
        else:
            v = torch.zeros_like(x[0].select(dirdim, d), dtype=F64)
        out.append(v)
    return torch.stack(out)


def _cur_act(act, frames):
    return torch.stack([act[frames[0]], act[frames[1]]])[:, :, None]         # [2,B,1]


def _zero(a, *xs):
    return [torch.where(a, x, torch.zeros_like(x)) for x in xs]


def _put(dst, frames, dirdim, src):
    for d, t in enumerate(frames):
        dst[t].select(dirdim, d).copy_(src[d])


# ------------------------------------------------------------------ LSTM

def lstm_forward(gx, whh, lens, forced=None, round_h=True, gx_mag=None, K=None):
    """pre = gx[t] + bf16(h_prev) . W_hh^T (i, f, g, o); c = f c_prev + i g; h = o tanh c; zeros and
    a reset state where t >= lens[b].  forced = (y_bf16, csave) of the kernel: h_prev is read from
    y_bf16[dir][t or t+2], c_prev from csave of the neighbouring frame (zero where inactive or
    outside).  gx_mag / K: sum of |terms| and their number when gx itself is a dot product
    (the fused input projection).  Returns dict gates, csave, y (before any rounding) and
    d_gates, d_csave, d_y."""
    T, B, _, H4 = gx.shape
    H = H4 // 4
    K = H if K is None else K
    wt = whh.to(F64).transpose(1, 2).contiguous()          # [2,H,4H]
    wabs = wt.abs().float()
    act = act_mask(T, lens)
    o = {k: torch.zeros(s, dtype=F64) for k, s in (
        ('gates', (T, 2, B, H, 4)), ('d_gates', (T, 2, B, H, 4)), ('csave', (T, 2, B, H)),
        ('d_csave', (T, 2, B, H)), ('y', (T, B, 2, H)), ('d_y', (T, B, 2, H)))}
    h = torch.zeros(2, B, H, dtype=F64)
    c = torch.zeros(2, B, H, dtype=F64)
    for s in range(T):
        cur, prv = (s, T - 1 - s), (s - 1, T - s)
        a = _cur_act(act, cur)
        if forced is not None:
            ybf, cs = forced
            hp = torch.stack([ybf[0, cur[0]], ybf[1, cur[1] + 2]]).to(F64)
            cp = _pick(cs, prv, 0, act)
        else:
            hp, cp = (bf16_round(h) if round_h else h), c
        g = _pick(gx, cur, 1)
        rec, mag = _dot(hp, wt, wabs)
        mag = mag + (g.abs() if gx_mag is None else _pick(gx_mag, cur, 1))
        pre = (g + rec).view(2, B, 4, H)
        dpre = ((K + 8) * U * mag).view(2, B, 4, H)
        gi, di = _sig(pre[:, :, 0], dpre[:, :, 0])
        gf, df = _sig(pre[:, :, 1], dpre[:, :, 1])
        gg, dg = _tanh(pre[:, :, 2], dpre[:, :, 2])
        go, do = _sig(pre[:, :, 3], dpre[:, :, 3])
        cn = gf * cp + gi * gg
        dc = cp.abs() * df + gg.abs() * di + gi * dg + di * dg + 2.0 ** -22 * ((gf * cp).abs() + (gi * gg).abs())
        tc, dtc = _tanh(cn, dc)
        hn = go * tc
        dh = tc.abs() * do + go * dtc + do * dtc + 2.0 ** -22 * hn.abs()
        gates, dgates = torch.stack([gi, gf, gg, go], -1), torch.stack([di, df, dg, do], -1)
        a4 = a[..., None]
        _put(o['gates'], cur, 0, torch.where(a4, gates, torch.zeros_like(gates)))
        _put(o['d_gates'], cur, 0, torch.where(a4, dgates, torch.zeros_like(gates)))
        hn, dh, cn, dc = _zero(a, hn, dh, cn, dc)
        _put(o['csave'], cur, 0, cn)
        _put(o['d_csave'], cur, 0, dc)
        _put(o['y'], cur, 1, hn)
        _put(o['d_y'], cur, 1, dh)
        h, c = hn, cn
    return o


def _dy_slab(dy, shared, frames):
    if shared:
        return torch.stack([dy[frames[0]], dy[frames[1]]]).to(F64)
    return torch.stack([dy[frames[0], :, 0], dy[frames[1], :, 1]]).to(F64)


def lstm_backward(dy, dy_shared, whhT, lens, gates, csave, forced=None, round_d=True):
    """dh = dy[t] + bf16(dgates_next) . W_hh with dgates_next the gate gradients of the frame
    processed just before (forced = the kernel's own dgates; zero at the start), then
        dc = dh o (1 - tanh^2 c) + dc_carry     d_o = dh tanh c  o (1 - o)
        d_i = dc g i (1 - i)    d_f = dc c_{t-1} f (1 - f)    d_g = dc i (1 - g^2)    dc_carry' = dc f
    from the saved gates, c_t and c_{t-1} (zero at an utterance's first frame).  dc_carry cannot
    be observed: it is carried here in fp64, with its radius, and is zero on padding frames.
    Returns dict dgates [T,B,2,4H], d_dgates."""
    T, B, H = dy.shape[0], dy.shape[1], dy.shape[-1]
    m = whhT.to(F64).transpose(1, 2).contiguous()          # [2,4H,H]
    mabs = m.abs().float()
    act = act_mask(T, lens)
    o = {k: torch.zeros(T, B, 2, 4 * H, dtype=F64) for k in ('dgates', 'd_dgates')}
    dgn = torch.zeros(2, B, 4 * H, dtype=F64)
    carry = torch.zeros(2, B, H, dtype=F64)
    dcarry = torch.zeros(2, B, H, dtype=F64)
    for s in range(T):
        cur, nxt, prv = (T - 1 - s, s), (T - s, s - 1), (T - 2 - s, s + 1)
        a = _cur_act(act, cur)
        if forced is not None:
            dgn = _pick(forced, nxt, 1, act)
        dyt = _dy_slab(dy, dy_shared, cur)
        rec, mag = _dot(dgn, m, mabs)
        dh = dyt + rec
        ddh = (4 * H + 8) * U * (mag + dyt.abs())
        g = _pick(gates, cur, 0)                            # [2,B,H,4]
        gi, gf, gg, go = g.unbind(-1)
        cs, cp = _pick(csave, cur, 0), _pick(csave, prv, 0, act)
        tc, dtc = _tanh(cs, torch.zeros_like(cs))
        omt = 1 - tc * tc
        domt = 2 * tc.abs() * dtc + dtc * dtc
        a1 = dh * go * omt
        da1 = go.abs() * (ddh * omt + dh.abs() * domt + ddh * domt)
        dc = a1 + carry
        ddc = da1 + dcarry + 2.0 ** -22 * (a1.abs() + carry.abs())
        oo = go * (1 - go)
        d_o = dh * tc * oo
        e_o = oo.abs() * (ddh * tc.abs() + dh.abs() * dtc + ddh * dtc)
        fi, ff, fg = gg * gi * (1 - gi), cp * gf * (1 - gf), gi * (1 - gg * gg)
        d = torch.stack([dc * fi, dc * ff, dc * fg, d_o], 2)            # [2,B,4,H]
        e = torch.stack([ddc * fi.abs(), ddc * ff.abs(), ddc * fg.abs(), e_o], 2) + 2.0 ** -20 * d.abs()
        a4 = a[..., None]
        d, e = torch.where(a4, d, torch.zeros_like(d)), torch.where(a4, e, torch.zeros_like(d))
        _put(o['dgates'], cur, 1, d.view(2, B, 4 * H))
        _put(o['d_dgates'], cur, 1, e.view(2, B, 4 * H))
        carry = dc * gf
        dcarry = ddc * gf.abs() + 2.0 ** -23 * carry.abs()
        carry, dcarry = _zero(a, carry, dcarry)
        if forced is None:
            dgn = d.view(2, B, 4 * H)
            dgn = bf16_round(dgn) if round_d else dgn
    return o


# ------------------------------------------------------------------ GRU

def gru_forward(gx, whh, lens, forced=None, round_h=True):
    """r = s(gx_r + h W_hr^T), z = s(gx_z + h W_hz^T), hn = h W_hn^T, n = tanh(gx_n + r hn),
    h' = (1 - z) n + z h with h rounded to bf16 inside the products only; records (r, z, n, hn).
    forced = (y_bf16, y) of the kernel: the operand of the products is read from y_bf16, the h of
    the last line from the fp32 y of the neighbouring frame.  Returns dict gates, y, d_gates, d_y."""
    T, B, _, H3 = gx.shape
    H = H3 // 3
    wt = whh.to(F64).transpose(1, 2).contiguous()          # [2,H,3H]
    wabs = wt.abs().float()
    act = act_mask(T, lens)
    o = {k: torch.zeros(s, dtype=F64) for k, s in (
        ('gates', (T, 2, B, H, 4)), ('d_gates', (T, 2, B, H, 4)), ('y', (T, B, 2, H)), ('d_y', (T, B, 2, H)))}
    h = torch.zeros(2, B, H, dtype=F64)
    for s in range(T):
        cur, prv = (s, T - 1 - s), (s - 1, T - s)
        a = _cur_act(act, cur)
        if forced is not None:
            ybf, y = forced
            hop = torch.stack([ybf[0, cur[0]], ybf[1, cur[1] + 2]]).to(F64)
            hp = _pick(y, prv, 1, act)
        else:
            hop, hp = (bf16_round(h) if round_h else h), h
        g = _pick(gx, cur, 1).view(2, B, 3, H)
        rec, mag = _dot(hop, wt, wabs)
        rec, mag = rec.view(2, B, 3, H), mag.view(2, B, 3, H)
        k = (H + 8) * U
        r, dr = _sig(g[:, :, 0] + rec[:, :, 0], k * (mag[:, :, 0] + g[:, :, 0].abs()))
        z, dz = _sig(g[:, :, 1] + rec[:, :, 1], k * (mag[:, :, 1] + g[:, :, 1].abs()))
        hn, dhn = rec[:, :, 2], k * mag[:, :, 2] + 2.0 ** -20 * rec[:, :, 2].abs()
        rhn = r * hn
        dnp = hn.abs() * dr + r * dhn + dr * dhn + 2.0 ** -22 * (g[:, :, 2].abs() + rhn.abs())
        n, dn = _tanh(g[:, :, 2] + rhn, dnp)
        hnew = (1 - z) * n + z * hp
        dh = ((1 - z) * dn + (hp - n).abs() * dz + dz * dn
              + 2.0 ** -22 * (((1 - z) * n).abs() + (z * hp).abs()) + 2.0 ** -20 * hnew.abs())
        gates, dgates = torch.stack([r, z, n, hn], -1), torch.stack([dr, dz, dn, dhn], -1)
        a4 = a[..., None]
        _put(o['gates'], cur, 0, torch.where(a4, gates, torch.zeros_like(gates)))
        _put(o['d_gates'], cur, 0, torch.where(a4, dgates, torch.zeros_like(gates)))
        hnew, dh = _zero(a, hnew, dh)
        _put(o['y'], cur, 1, hnew)
        _put(o['d_y'], cur, 1, dh)
        h = hnew
    return o


def gru_backward(dy, dy_shared, whhT, lens, gates, y, forced=None, round_d=True):
    """dh = dy[t] + carry + bf16([dr, dz, dhn]) . W_hh of the frame processed just before
    (forced = the kernel's own (dgx, dhn)), then
        dn = dh (1 - z)(1 - n^2)   dr = dn hn r (1 - r)   dz = dh (h_prev - n) z (1 - z)
        dhn = dn r   carry' = dh z
    with h_prev the fp32 y of the neighbouring frame (zero where inactive).  Returns dict
    dgx [T,B,2,3H] = (dr, dz, dn), dhn [T,B,2,H], d_dgx, d_dhn."""
    T, B, H = dy.shape[0], dy.shape[1], dy.shape[-1]
    m = whhT.to(F64).transpose(1, 2).contiguous()          # [2,3H,H]
    mabs = m.abs().float()
    act = act_mask(T, lens)
    o = {'dgx': torch.zeros(T, B, 2, 3 * H, dtype=F64), 'd_dgx': torch.zeros(T, B, 2, 3 * H, dtype=F64),
         'dhn': torch.zeros(T, B, 2, H, dtype=F64), 'd_dhn': torch.zeros(T, B, 2, H, dtype=F64)}
    op = torch.zeros(2, B, 3 * H, dtype=F64)
    carry = torch.zeros(2, B, H, dtype=F64)
    dcarry = torch.zeros(2, B, H, dtype=F64)
    for s in range(T):
        cur, nxt, prv = (T - 1 - s, s), (T - s, s - 1), (T - 2 - s, s + 1)
        a = _cur_act(act, cur)
        if forced is not None:
            op = torch.cat([_pick(forced[0], nxt, 1, act)[:, :, :2 * H], _pick(forced[1], nxt, 1, act)], -1)
        dyt = _dy_slab(dy, dy_shared, cur)
        rec, mag = _dot(op, m, mabs)
        dh = dyt + carry + rec
        ddh = (3 * H + 8) * U * (mag + dyt.abs() + carry.abs()) + dcarry
        r, z, n, hn = _pick(gates, cur, 0).unbind(-1)
        hp = _pick(y, prv, 1, act)
        fn = (1 - z) * (1 - n * n)
        dn, e_n = dh * fn, ddh * fn.abs()
        fr, fz = hn * r * (1 - r), (hp - n) * z * (1 - z)
        d = torch.stack([dn * fr, dh * fz, dn, dn * r], 2)              # [2,B,4,H]
        e = torch.stack([e_n * fr.abs(), ddh * fz.abs(), e_n, e_n * r.abs()], 2) + 2.0 ** -20 * d.abs()
        a4 = a[..., None]
        d, e = torch.where(a4, d, torch.zeros_like(d)), torch.where(a4, e, torch.zeros_like(d))
        _put(o['dgx'], cur, 1, d[:, :, :3].reshape(2, B, 3 * H))
        _put(o['d_dgx'], cur, 1, e[:, :, :3].reshape(2, B, 3 * H))
        _put(o['dhn'], cur, 1, d[:, :, 3])
        _put(o['d_dhn'], cur, 1, e[:, :, 3])
        carry = dh * z
        dcarry = ddh * z.abs() + 2.0 ** -23 * carry.abs()
        carry, dcarry = _zero(a, carry, dcarry)
        if forced is None:
            op = torch.cat([d[:, :, 0], d[:, :, 1], d[:, :, 3]], -1)
            op = bf16_round(op) if round_d else op
    return o


# ------------------------------------------------------------------ judging a set of outputs

class Verdict(object):
    """violations of the rule over the outputs of one call; `add` one output at a time"""

    def __init__(self):
        self.count, self.checked, self.worst, self.max_ulp, self.lines = 0, 0, None, 0.0, []
        self.tight, self.tiny = 0, 0

    def add(self, name, got, want, delta, bf16, mask=None, where=None):
        """mask: elements to check (broadcastable bool; default all).  where(index tuple) -> the
        (t, b, dir, gate, j) of an element, for the report."""
        bad = violations(got, want, delta, bf16)
        m = torch.ones_like(bad) if mask is None else mask.expand_as(bad)
        bad = bad & m
        n = int(m.sum())
        self.checked += n
        ue = torch.where(m & (want.abs() >= TINY), ulp_error(got, want), torch.zeros_like(want))
        ue = torch.nan_to_num(ue, nan=float('inf'))
        self.max_ulp = max(self.max_ulp, float(ue.max()) if ue.numel() else 0.0)
        self.tight += int((m & (delta < 0.25 * bf16_ulp(want))).sum())
        self.tiny += int((m & (want.abs() < TINY)).sum())
        k = int(bad.sum())
        if k:
            self.count += k
            i = int(torch.where(bad, ue, -torch.ones_like(ue)).argmax())
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), bad.shape))
            self.lines.append('%s: %d of %d violate; worst at %s: got %r want %r delta %.3g (%.2f ulp)' % (
                name, k, n, where(idx) if where else idx, float(got.to(F64)[idx]), float(want[idx]),
                float(delta[idx]), float(ue[idx])))

    def report(self):
        return '%d of %d elements violate\n' % (self.count, self.checked) + '\n'.join(self.lines)


def _w_gates(i):        # gates / csave index [t, dir, b, j(, gate)]
    return dict(t=i[0], dir=i[1], b=i[2], j=i[3], gate=i[4] if len(i) > 4 else None)


def _w_y(i):            # y [t, b, dir, j]
    return dict(t=i[0], b=i[1], dir=i[2], j=i[3], gate=None)


def _w_dg(H):           # dgates [t, b, dir, gate*H + j]
    return lambda i: dict(t=i[0], b=i[1], dir=i[2], gate=i[3] // H, j=i[3] % H)


def judge_lstm_forward(v, want, y, y_bf16, gates, csave, lens):
    T = y.shape[0]
    act = act_mask(T, lens)
    v.add('gates', gates, want['gates'], want['d_gates'], True, act[:, None, :, None, None], _w_gates)
    v.add('csave', csave, want['csave'], want['d_csave'], False, act[:, None, :, None], _w_gates)
    v.add('y', y, want['y'], want['d_y'], False, act[:, :, None, None], _w_y)
    _structure(v, y, y_bf16, act)


def judge_gru_forward(v, want, y, y_bf16, gates, lens):
    T = y.shape[0]
    act = act_mask(T, lens)
    v.add('gates', gates, want['gates'], want['d_gates'], True, act[:, None, :, None, None], _w_gates)
    v.add('y', y, want['y'], want['d_y'], False, act[:, :, None, None], _w_y)
    _structure(v, y, y_bf16, act)


def _structure(v, y, y_bf16, act):
    """padding frames of y are exact zeros; y_bf16 is bf16(y) between two zero frames; no NaN"""
    T = y.shape[0]
    pad = ~act[:, :, None, None].expand_as(y)
    bad = int((y[pad] != 0).sum()) + int(torch.isnan(y).sum())
    want = torch.zeros_like(y_bf16)
    want[:, 1:T + 1] = y.to(torch.bfloat16).permute(2, 0, 1, 3)
    bad_bf = int((y_bf16.view(torch.int16) != want.view(torch.int16)).sum())
    if bad:
        v.count += bad
        v.lines.append('y: %d padding elements are not exact zeros (or NaN)' % bad)
    if bad_bf:
        v.count += bad_bf
        v.lines.append('y_bf16: %d elements are not bf16(y) between two zero frames' % bad_bf)


def judge_backward(v, want, outs, lens, H):
    """outs: {'dgates': t} or {'dgx': t, 'dhn': t}; padding frames must be exact zeros"""
    for name, got in outs.items():
        T = got.shape[0]
        act = act_mask(T, lens)
        v.add(name, got, want[name], want['d_' + name], True, act[:, :, None, None], _w_dg(H))
        pad = ~act[:, :, None, None].expand_as(got)
        g = got.to(F64)
        bad = int((g[pad] != 0).sum()) + int(torch.isnan(g).sum())
        if bad:
            v.count += bad
            v.lines.append('%s: %d padding elements are not exact zeros (or NaN)' % (name, bad))


# ------------------------------------------------------------------ inputs and the case matrix

def make_lens(kind, T, B, gen):
    """descending, as the callers pass it"""
    if kind == 'full':
        lens = torch.full((B,), T)
    elif kind == 'ragged':
        lens = torch.randint(1, T + 1, (B,), generator=gen).sort(descending=True)[0]
        lens[0] = T
    elif kind == 'one_long':
        lens = torch.ones(B, dtype=torch.int64)
        lens[0] = T
    elif kind == 'stair':       # one frame less per utterance, across the 32-row tile boundaries
        lens = (T - (torch.arange(B) - min(24, B // 2)).clamp(min=0)).clamp(min=1)
    else:
        raise ValueError(kind)
    return lens.to(torch.int64)


GARBAGE = 3e4


def quiet(H):
    """(gx_scale, w_scale) of the quiet draw: gx ~ 0.8 N(0,1), W_hh ~ N(0,1) / (2H).  With weights
    that shrink like 1/H, not 1/sqrt(H), the sum of |a_k b_k| over the K terms of a recurrent
    product does not grow with H, so the worst-case radius (K + 8) 2^-24 sum|a_k b_k| stays small
    beside the addend (gx, dy) at every hidden size; |gx| rarely reaches the 3.1 where tanh
    becomes exactly 1 in bf16."""
    return 0.8, 0.5 / H ** 0.5


def make_inputs(rnn, T, B, H, kind, seed, gx_scale=1.5, dy_shared=False, w_scale=1.0):
    """gx ~ gx_scale N(0,1), W_hh ~ w_scale N(0,1)/sqrt(H) (bf16), dy ~ N(0,1) with a block of exact
    zeros, large finite garbage in gx and dy on padding frames.  Three draws are used: the base one
    (1.5, 1), the saturated one (6, 1: bf16 records that are exactly 0, 1 or -1) and the quiet one
    (quiet(H): few saturated records and a recurrent term small beside its addend, where the
    radius stays under a quarter bf16 ulp; see test_radius_is_below_a_quarter_ulp_on_95_percent).
    The base and saturated draws are the ones that load the recurrent product; the quiet draw
    judges the cell arithmetic with the tightest radius."""
    G = 4 if rnn == 'lstm' else 3
    gen = torch.Generator().manual_seed(seed)
    lens = make_lens(kind, T, B, gen)
    gx = torch.randn(T, B, 2, G * H, generator=gen) * gx_scale
    whh = (w_scale * torch.randn(2, G * H, H, generator=gen) / H ** 0.5).to(torch.bfloat16)
    dy = torch.randn(*((T, B, H) if dy_shared else (T, B, 2, H)), generator=gen)
    if T >= 4:
        dy[T // 3:T // 2 + 1, 3::16] = 0
    else:
        dy[0, 0, ..., 0] = 0
    pad = ~act_mask(T, lens)
    sign = torch.sign(torch.randn(T, B, generator=gen))
    gx[pad] = (GARBAGE * sign[pad])[:, None, None]
    dy[pad] = (GARBAGE * sign[pad]).view(-1, *([1] * (dy.dim() - 2)))
    return dict(lens=lens, gx=gx, whh=whh, whhT=whh.transpose(1, 2).contiguous(), dy=dy)


def synthetic_saved(rnn, T, B, H, lens, seed):
    """saved tensors a forward pass would rarely produce.  LSTM: gates uniform in the open
    interval ((-1, 1) for g) rounded to bf16, the exact values 0 and 1 (-1) among them, csave ~
    3 N(0,1).  GRU: records (r, z, n, hn) likewise with hn ~ N(0,1), and y ~ U(-1, 1)."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(T, 2, B, H, 4, generator=gen)
    edge = torch.rand(T, 2, B, H, 4, generator=gen)
    u = torch.where(edge < 0.02, torch.zeros_like(u), torch.where(edge > 0.98, torch.ones_like(u), u))
    u[..., 2] = 2 * u[..., 2] - 1
    if rnn == 'gru':
        u[..., 3] = torch.randn(T, 2, B, H, generator=gen)
    gates = u.to(torch.bfloat16)
    act = act_mask(T, lens)
    if rnn == 'lstm':
        return gates, 3 * torch.randn(T, 2, B, H, generator=gen)
    y = (2 * torch.rand(T, B, 2, H, generator=gen) - 1) * act[:, :, None, None]
    return gates, y


def case(rnn, T, B, H, kind, gx_bf16=False, dy_shared=False, persist=True, gx_scale=1.5, fused=False,
         w_scale=1.0):
    return dict(rnn=rnn, T=T, B=B, H=H, kind=kind, gx_bf16=gx_bf16, dy_shared=dy_shared, persist=persist,
                gx_scale=gx_scale, fused=fused, w_scale=w_scale)


def case_id(c):
    return '%s-T%d-B%d-H%d-%s%s%s%s%s%s' % (
        c['rnn'], c['T'], c['B'], c['H'], c['kind'], '-gxbf16' if c['gx_bf16'] else '',
        '-dyshared' if c['dy_shared'] else '', '' if c['persist'] else '-perstep',
        {1.5: '', 6.0: '-sat', 0.8: '-quiet'}[c['gx_scale']], '-fused' if c['fused'] else '')


def _matrix():
    """Every value of every axis, and every hidden size with each kind of lens; the other axes
    rotate over the cases (B, T, gx type, dy form, launch form, input scale)."""
    kinds = ('full', 'ragged', 'one_long', 'stair')
    bs = (1, 31, 32, 33, 63, 64, 65, 96)
    ts = (23, 40, 2, 1, 23, 40)
    out, n = [], 0
    for rnn, hs in (('lstm', (64, 128, 256, 320, 384, 512, 768)), ('gru', (64, 128, 256, 320))):
        for H in hs:
            for kind in kinds:
                B, T = bs[n % len(bs)], ts[n % len(ts)]
                if kind == 'stair':         # needs a tile boundary and frames to step down over
                    B, T = (33, 65, 96, 63)[n % 4], (23, 40)[n % 2]
                gs, ws = ((1.5, 1.0), (1.5, 1.0), quiet(H), (1.5, 1.0), (6.0, 1.0))[n % 5]
                out.append(case(rnn, T, B, H, kind, gx_bf16=n % 2 == 1, dy_shared=n % 4 >= 2,
                                persist=n % 3 != 2, gx_scale=gs, w_scale=ws))
                n += 1
    for rnn in ('lstm', 'gru'):
        out += [case(rnn, 23, 512, 64, 'ragged', gx_bf16=True),
                case(rnn, 40, 900, 320, 'ragged', dy_shared=True),
                case(rnn, 334, 512, 320, 'ragged', gx_bf16=True, dy_shared=True)]
    out += [case('lstm', 40, 512, 320, 'stair', persist=False),
            case('lstm', 23, 65, 64, 'ragged', fused=True), case('lstm', 40, 33, 128, 'stair', fused=True),
            case('lstm', 2, 96, 256, 'one_long', fused=True), case('lstm', 41, 64, 320, 'ragged', fused=True)]
    return out


CASES = _matrix()


def fused_inputs(T, B, H, kind, seed):
    """x [T,B,H] bf16 and W_ih [8H,H] bf16 for the fused input projection (F = H), with gx = x W_ih^T
    formed in fp64 from the same bf16 operands and the sum of |terms| for the radius"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, H, generator=gen).to(torch.bfloat16)
    wih = (1.5 * torch.randn(8 * H, H, generator=gen) / H ** 0.5).to(torch.bfloat16)
    gx = (x.to(F64).view(T * B, H) @ wih.to(F64).t()).view(T, B, 2, 4 * H)
    mag = (x.float().abs().view(T * B, H) @ wih.float().abs().t()).double().view(T, B, 2, 4 * H) * (1 + 1e-5)
    return x, wih, gx, mag
