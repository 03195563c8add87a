// Dynamic programmes over a batch of pruned lattices that stays on the device (include/asr_amd.h:
// asr_lattice_bestpath_f64, asr_lattice_posterior_f64, asr_lattice_nbest_f64, asr_lattice_mbr_f64 and their
// _supported / _workspace_bytes).
//
// The lattices are those of asr_wfst_lattice_f32 in the canonical form of DESIGN.md section 4.20,
// laid end to end: nodes by (utterance, time, state), arcs by (utterance, source node, graph arc).
// A node's level is (time, epsilon rank of its state); every arc rises in level, so a node's value
// is final once the levels below it (tropical sweep, forward) or above it (backward) are done.
//
//   bestpath   one workgroup per (scale pair, utterance), persistent over the utterance's levels.
//              A lane owns a node and walks its in-arcs in the stored order: cost(v) = min over
//              in-arcs of cost(u) + x, x = fl(fl(lm w) - fl(sc lp)) in fp64 without contraction,
//              the back-pointer the in-arc of the smallest GRAPH arc index among those that attain
//              the minimum.  Then the end node (smallest index among the minima of cost + lm end)
//              and the traceback by one lane.  IEEE semantics as numpy's: a NaN anywhere in the
//              utterance's costs (0 * inf, inf - inf) leaves it without a path.
//   posterior  one workgroup per utterance: forward over the levels upwards (in-arcs), backward
//              downwards (out-arcs), each node reduced by its one owner lane as max-then-sum
//              logsumexp in the stored order; no atomics, so two runs give the same bits.
//   nbest      one workgroup per utterance, levels downwards: a wave owns a node and merges the lists of
//              its out-arcs' destinations, a lane per arc, into the node's n cheapest distinct word
//              suffixes by wave-wide minima of a five-field key; then a lane per entry of the start
//              node walks its chain forwards.  Defined by a total order, so two runs give the same bits.
//   mbr        one workgroup per utterance, all iterations in one launch: a wave owns a node, its lanes the
//              hypothesis slots; expected edit distances upwards, masses downwards, in 64-bit fixed point, so
//              that sums commute and integer atomics are legal; then every slot takes its heaviest word.
//
// All synchronise with workgroup barriers only.  Every node, arc, level and graph index read from
// memory is range-checked before it is used (the tensors may come from a caller): a violation raises
// the utterance's status word and ends its workgroup.  Every loop is bounded by the counts passed in.
// The batch's header struct, those checks, the arithmetic of an arc and the host validation are csrc/lattice_batch.h's.
#include "common.h"
#include "lattice_batch.h"

namespace {

struct BestArgs {
    Lat t;
    int P;
    const double *ac_scale, *lm_scale;      // [P]; ac_scale NaN: the utterance's own
    double *cost;                           // workspace [P][nodes of the launch]
    int32_t *bp;
    int64_t n_launch;
    double *out_cost;                       // [P][B][3]
    int32_t *out_nwords, *out_words, *out_status;       // [P][B], [P][L], [P][B]
};

template <int NT>
__global__ __launch_bounds__(NT) void lattice_bestpath_kernel(const BestArgs q) {
    const Lat &t = q.t;
    const int tid = threadIdx.x;
    const int b = t.b_begin + (int)(blockIdx.x % (unsigned)t.b_count);
    const int pr = (int)(blockIdx.x / (unsigned)t.b_count);
    __shared__ int s_bad, s_nan;
    __shared__ double s_val[NT];
    __shared__ int64_t s_idx[NT];
    if (tid == 0) s_bad = 0, s_nan = 0;
    __syncthreads();
    const int64_t o = (int64_t)pr * t.B + b;
    const Span sp = span_of(t, b);
    const int64_t nlev = sp.l1 - sp.l0;
    if (!sp.ok || !levels_cover(t, sp)) {       // uniform: every lane read the same words
        if (tid == 0) {
            q.out_cost[3 * o] = q.out_cost[3 * o + 1] = q.out_cost[3 * o + 2] = DINF;
            q.out_nwords[o] = 0;
            q.out_status[o] = 1;
        }
        return;
    }
    const double sc = scale_of(t, b, q.ac_scale[pr]);
    const double lm = q.lm_scale[pr];
    double *const cost = q.cost + (int64_t)pr * q.n_launch - t.n_begin;        // indexed by batch node
    int32_t *const bp = q.bp + (int64_t)pr * q.n_launch - t.n_begin;
    bool bad = false, nan = false, dead = false;
    for (int64_t l = sp.l0; l < sp.l1; ++l) {
        const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
        if (!level_range(e0, e1, sp.n0, sp.n1)) {
            bad = true;
        } else {
            for (int64_t e = e0 + tid; e < e1; e += NT) {
                int64_t v, j0, j1;
                if (!node_at(t, sp, e, l, v)) {
                    bad = true;
                    continue;
                }
                const bool is_start = t.time[v] == 0 && t.state[v] == t.start;
                double c = is_start ? 0.0 : DINF;
                int64_t best_g = INT64_MAX;
                int32_t back = -1;
                if (!in_arcs_of(t, sp, v, j0, j1)) {
                    bad = true;
                    continue;
                }
                for (int64_t j = j0; j < j1; ++j) {
                    int64_t a, u, g;
                    if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
                        bad = true;
                        break;
                    }
                    const double cand = cost[u] + arc_cost(lm, sc, t.w[g], t.lp[a]);
                    if (cand != cand) {
                        nan = true;
                    } else if (cand < c) {
                        c = cand, best_g = g, back = (int32_t)(a - sp.a0);
                    } else if (cand == c && cand < DINF && g <= best_g) {
                        best_g = g, back = (int32_t)(a - sp.a0);
                    }
                }
                cost[v] = c;
                bp[v] = is_start ? -1 : back;
            }
        }
        dead = __syncthreads_or(bad) != 0;      // also makes the level's costs visible to every lane
        if (dead) break;
    }
    // the end node: the smallest index among the minima of cost + lm * end
    double m = DINF;
    int64_t mi = -1;
    const int frames = t.frames[b], reached = t.reached[b];
    if (!dead) {
        for (int64_t v = sp.n0 + tid; v < sp.n1; v += NT) {
            const double e = end_cost(t, v, frames, reached, bad);
            const double tot = cost[v] + lm * e;
            if (tot != tot)
                nan = true;
            else if (tot < m)
                m = tot, mi = v;
        }
    }
    s_val[tid] = m;
    s_idx[tid] = mi;
    if (bad || dead) s_bad = 1;
    if (nan) s_nan = 1;
    __syncthreads();
    if (tid != 0) return;
    double gc = DINF, ac = DINF;
    int nw = 0;
    m = DINF, mi = -1;
    if (!s_bad && !s_nan) {
        for (int i = 0; i < NT; ++i)
            if (s_idx[i] >= 0 && (s_val[i] < m || (s_val[i] == m && s_idx[i] < mi))) m = s_val[i], mi = s_idx[i];
    }
    if (mi >= 0) {
        const double e = end_cost(t, mi, frames, reached, bad);
        gc = e < DINF ? e : 0.0;
        ac = 0.0;
        int32_t *const words = q.out_words + (int64_t)pr * t.L + sp.l0;
        int64_t cur = mi;
        for (int64_t step = 0; step <= nlev; ++step) {      // a path has at most one arc per level
            const int32_t back = bp[cur];
            if (back < 0) break;
            int64_t a, u, g;
            if (!back_arc_at(t, sp, back, cur, a, u, g)) {
                bad = true;
                break;
            }
            gc += (double)t.w[g];
            ac -= (double)t.lp[a];
            const int32_t word = t.ol[g];
            if (word != 0) {
                if (nw >= nlev) {
                    bad = true;
                    break;
                }
                words[nw++] = word;
            }
            cur = u;
        }
        for (int i = 0, j = nw - 1; i < j; ++i, --j) {      // gathered end to start: path order
            const int32_t x = words[i];
            words[i] = words[j];
            words[j] = x;
        }
    }
    const bool none = mi < 0 || bad || s_bad;
    q.out_cost[3 * o] = none ? DINF : m;
    q.out_cost[3 * o + 1] = none ? DINF : gc;
    q.out_cost[3 * o + 2] = none ? DINF : ac;
    q.out_nwords[o] = none ? 0 : nw;
    q.out_status[o] = (bad || s_bad) ? 1 : 0;
}

struct PostArgs {
    Lat t;
    double ac_scale, lm_scale;              // ac_scale NaN: the utterance's own
    double *fwd, *bwd;                      // workspace [nodes of the launch]
    double *log_z, *arc_post, *node_post;   // [B], [A], [N]
    int32_t *out_status;                    // [B]
};

template <int NT>
__global__ __launch_bounds__(NT) void lattice_posterior_kernel(const PostArgs q) {
    const Lat &t = q.t;
    const int tid = threadIdx.x;
    const int b = t.b_begin + (int)blockIdx.x;
    __shared__ int64_t s_start;
    if (tid == 0) s_start = INT64_MAX;
    __syncthreads();
    const Span sp = span_of(t, b);
    if (!sp.ok || !levels_cover(t, sp)) {
        if (tid == 0) q.log_z[b] = -DINF, q.out_status[b] = 1;
        return;
    }
    const double sc = scale_of(t, b, q.ac_scale);
    const double lm = q.lm_scale;
    double *const fwd = q.fwd - t.n_begin, *const bwd = q.bwd - t.n_begin;
    const int frames = t.frames[b], reached = t.reached[b];
    bool bad = false, dead = false;
    // forward, levels upwards
    for (int64_t l = sp.l0; l < sp.l1; ++l) {
        const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
        if (!level_range(e0, e1, sp.n0, sp.n1)) {
            bad = true;
        } else {
            for (int64_t e = e0 + tid; e < e1; e += NT) {
                int64_t v, j0, j1;
                if (!node_at(t, sp, e, l, v)) {
                    bad = true;
                    continue;
                }
                const bool is_start = t.time[v] == 0 && t.state[v] == t.start;
                if (is_start) atomicMin((unsigned long long *)&s_start, (unsigned long long)v);
                if (!in_arcs_of(t, sp, v, j0, j1)) {
                    bad = true;
                    continue;
                }
                double m = is_start ? 0.0 : -DINF, s = 0.0;
                for (int pass = 0; pass < 2 && !bad; ++pass) {
                    if (pass == 1) {
                        if (m == -DINF) break;
                        s = is_start ? exp(0.0 - m) : 0.0;
                    }
                    for (int64_t j = j0; j < j1; ++j) {
                        int64_t a, u, g;
                        if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
                            bad = true;
                            break;
                        }
                        const double term = log_times(fwd[u], arc_cost(lm, sc, t.w[g], t.lp[a]));
                        if (pass == 0)
                            m = term > m ? term : m;
                        else if (term != -DINF)
                            s += exp(term - m);
                    }
                }
                fwd[v] = lse_value(m, s);
            }
        }
        dead = __syncthreads_or(bad) != 0;
        if (dead) break;
    }
    // backward, levels downwards
    if (!dead) {
        for (int64_t l = sp.l1 - 1; l >= sp.l0; --l) {
            const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];     // checked in the forward
            for (int64_t e = e0 + tid; e < e1; e += NT) {
                const int64_t v = t.level_node[e];
                int64_t j0, j1;
                const double en = end_cost(t, v, frames, reached, bad);
                const double stop = en < DINF ? 0.0 - lm * en : -DINF;
                if (!out_arcs_of(t, sp, v, j0, j1)) {
                    bad = true;
                    continue;
                }
                double m = stop, s = 0.0;
                for (int pass = 0; pass < 2 && !bad; ++pass) {
                    if (pass == 1) {
                        if (m == -DINF) break;
                        s = stop != -DINF ? exp(stop - m) : 0.0;
                    }
                    for (int64_t a = j0; a < j1; ++a) {
                        int64_t d, g;
                        if (!out_arc_at(t, sp, a, v, l, d, g)) {
                            bad = true;
                            break;
                        }
                        const double term = log_times(bwd[d], arc_cost(lm, sc, t.w[g], t.lp[a]));
                        if (pass == 0)
                            m = term > m ? term : m;
                        else if (term != -DINF)
                            s += exp(term - m);
                    }
                }
                bwd[v] = lse_value(m, s);
            }
            dead = __syncthreads_or(bad) != 0;
            if (dead) break;
        }
    }
    const int64_t st = s_start;
    const double z = (!dead && st >= sp.n0 && st < sp.n1) ? bwd[st] : -DINF;
    for (int64_t v = sp.n0 + tid; v < sp.n1; v += NT) {
        double r = -DINF;
        if (z != -DINF && fwd[v] != -DINF && bwd[v] != -DINF) r = fwd[v] + bwd[v] - z;
        q.node_post[v] = r;
    }
    for (int64_t a = sp.a0 + tid; a < sp.a1; a += NT) {
        double r = -DINF;
        if (z != -DINF) {
            int64_t u, d, g;
            if (!arc_at(t, sp, a, u, d, g)) {
                bad = true;                     // an arc that no node's range covered
            } else {
                const double part = log_times(fwd[u], arc_cost(lm, sc, t.w[g], t.lp[a]));
                if (part != -DINF && bwd[d] != -DINF) r = part + bwd[d] - z;
            }
        }
        q.arc_post[a] = r;
    }
    dead = __syncthreads_or(bad) != 0 || dead;
    if (tid == 0) q.log_z[b] = z, q.out_status[b] = dead ? 1 : 0;
}

// ---- n-best lists (asr_lattice_nbest_f64) --------------------------------
// A list entry is 28 bytes of workspace: cost f64, suffix hash u64, word count, out-arc and rank i32;
// a node has n entries and one i32 count.  One wave owns a node; a lane owns an out-arc of it (64 arcs
// a round) and, of the list under construction, the entry of its own index: hence n <= 64.
constexpr int NBEST_MAX = 64;
constexpr uint64_t NBEST_HASH_MUL = 0x9E3779B97F4A7C15ull;

struct NbestArgs {
    Lat t;
    int n;
    double ac_scale, lm_scale;              // ac_scale NaN: the utterance's own
    double *ec;                             // workspace: [nodes of the launch][n] each, ecnt [nodes]
    uint64_t *eh;
    int32_t *elen, *earc, *erank, *ecnt;
    int32_t *out_count;                     // [B]
    double *out_cost;                       // [B][n]
    int32_t *out_nwords, *out_words, *out_status;       // [B][n], [n L], [B]
};

// the order of the candidates: (cost, words, hash, (arc + 1, rank)); costs are never NaN here
struct NKey {
    double c;
    uint64_t h, ar;
    int32_t len, valid;
};

__device__ __forceinline__ bool key_less(const NKey &a, const NKey &b) {
    if (a.c != b.c) return a.c < b.c;
    if (a.len != b.len) return a.len < b.len;
    if (a.h != b.h) return a.h < b.h;
    return a.ar < b.ar;
}

__device__ __forceinline__ NKey key_from_lane(const NKey &k, int src) {
    NKey o;
    o.c = __shfl(k.c, src);
    o.h = (uint64_t)__shfl((unsigned long long)k.h, src);
    o.ar = (uint64_t)__shfl((unsigned long long)k.ar, src);
    o.len = __shfl(k.len, src);
    o.valid = __shfl(k.valid, src);
    return o;
}

// the smallest valid key of the wave, in every lane
__device__ __forceinline__ NKey wave_min(NKey k) {
    for (int m = 1; m < 64; m <<= 1) {
        NKey o;
        o.c = __shfl_xor(k.c, m);
        o.h = (uint64_t)__shfl_xor((unsigned long long)k.h, m);
        o.ar = (uint64_t)__shfl_xor((unsigned long long)k.ar, m);
        o.len = __shfl_xor(k.len, m);
        o.valid = __shfl_xor(k.valid, m);
        if (o.valid && (!k.valid || key_less(o, k))) k = o;
    }
    return k;
}

template <int NT>
__global__ __launch_bounds__(NT) void lattice_nbest_kernel(const NbestArgs q) {
    const Lat &t = q.t;
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = t.b_begin + (int)blockIdx.x;
    const int n = q.n;
    __shared__ unsigned long long s_start;
    if (tid == 0) s_start = ~0ull;
    __syncthreads();
    const Span sp = span_of(t, b);
    if (!sp.ok || !levels_cover(t, sp)) {
        if (tid == 0) q.out_count[b] = 0, q.out_status[b] = 1;
        return;
    }
    const double sc = scale_of(t, b, q.ac_scale);
    const double lm = q.lm_scale;
    const int frames = t.frames[b], reached = t.reached[b];
    const int64_t nlev = sp.l1 - sp.l0;
    double *const ec = q.ec - t.n_begin * n;            // indexed by batch node * n + rank
    uint64_t *const eh = q.eh - t.n_begin * n;
    int32_t *const elen = q.elen - t.n_begin * n, *const earc = q.earc - t.n_begin * n;
    int32_t *const erank = q.erank - t.n_begin * n, *const ecnt = q.ecnt - t.n_begin;
    bool bad = false, dead = false;
    for (int64_t l = sp.l1 - 1; l >= sp.l0; --l) {      // levels downwards: the lists above are final
        const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
        if (!level_range(e0, e1, sp.n0, sp.n1)) {
            bad = true;
        } else {
            for (int64_t e = e0 + wave; e < e1; e += NW) {      // everything here is uniform in the wave
                int64_t v, j0, j1;
                if (!node_at(t, sp, e, l, v)) {
                    bad = true;
                    continue;
                }
                if (lane == 0 && t.time[v] == 0 && t.state[v] == t.start) atomicMin(&s_start, (unsigned long long)v);
                if (!out_arcs_of(t, sp, v, j0, j1)) {
                    bad = true;
                    continue;
                }
                // the list so far: entry i in lane i.  It starts as the stop entry alone.
                NKey cur;
                cur.c = scaled_end(t, v, frames, reached, lm, bad);
                cur.h = 0, cur.ar = 0, cur.len = 0;
                int m = cur.c < DINF ? 1 : 0;
                cur.valid = lane < m;
                for (int64_t jb = j0; jb < j1; jb += 64) {      // 64 out-arcs a round against that list
                    const int64_t a = jb + lane;
                    bool has = a < j1;
                    double x = DINF;
                    int32_t olab = 0;
                    int64_t dbase = 0;
                    int dcnt = 0, lo = 0;
                    if (has) {
                        int64_t d, g;
                        if (!out_arc_at(t, sp, a, v, l, d, g)) {        // the level must rise: list(d) is final
                            bad = true, has = false;
                        } else {
                            x = arc_cost(lm, sc, t.w[g], t.lp[a]);
                            olab = t.ol[g];
                            dcnt = ecnt[d];
                            dbase = d * n;
                            if (dcnt < 0 || dcnt > n) bad = true, has = false;
                            if (!(x < DINF)) has = false;       // +inf or NaN: no candidate survives
                        }
                    }
                    const uint64_t arhi = (uint64_t)(a - sp.a0 + 1) << 32;
                    NKey last, best;
                    last.valid = 0, best.valid = 0;
                    // this arc's smallest candidate above `last`.  c' = fl(x + c_r) does not fall as r
                    // grows, so the ranks whose c' is below last.c are spent for good (lo), and the scan
                    // ends at the first c' above the best so far; equal c' are compared in full.
                    auto rescan = [&]() {
                        best.valid = 0;
                        for (int r = lo; r < dcnt; ++r) {
                            const double c = x + ec[dbase + r];
                            if (!(c < DINF)) break;
                            if (last.valid && c < last.c) {
                                lo = r + 1;
                                continue;
                            }
                            if (best.valid && c > best.c) break;
                            NKey k;
                            k.c = c;
                            k.len = elen[dbase + r] + (olab != 0 ? 1 : 0);
                            const uint64_t h = eh[dbase + r];
                            k.h = olab != 0 ? h * NBEST_HASH_MUL + (uint64_t)(int64_t)olab + 1 : h;
                            k.ar = arhi | (uint32_t)r;
                            k.valid = 1;
                            if (last.valid && !key_less(last, k)) continue;
                            if (!best.valid || key_less(k, best)) best = k;
                        }
                    };
                    if (has) rescan();
                    NKey out;                   // the merged list: entry i in lane i
                    out.c = DINF, out.h = 0, out.ar = 0, out.len = 0, out.valid = 0;
                    int mo = 0, po = 0;
                    for (int it = 0; it < 65 * n && mo < n; ++it) {     // every turn spends a candidate
                        NKey w = wave_min(best);
                        bool old = false;
                        if (po < m) {
                            const NKey head = key_from_lane(cur, po);
                            if (!w.valid || key_less(head, w)) w = head, old = true;
                        }
                        if (!w.valid) break;
                        last = w;
                        if (old)
                            ++po;
                        else if (has && best.valid && best.ar == w.ar)
                            rescan();
                        const bool dup = lane < mo && out.len == w.len && out.h == w.h;
                        if (__ballot(dup) == 0ull) {
                            if (lane == mo) out = w;
                            ++mo;
                        }
                    }
                    cur = out, m = mo;
                }
                if (lane < m) {
                    const int64_t i = v * n + lane;
                    ec[i] = cur.c, eh[i] = cur.h, elen[i] = cur.len;
                    earc[i] = (int32_t)(cur.ar >> 32) - 1;
                    erank[i] = (int32_t)(cur.ar & 0xFFFFFFFFull);
                }
                if (lane == 0) ecnt[v] = m;
            }
        }
        dead = __syncthreads_or(bad) != 0;      // also makes the level's lists visible to every wave
        if (dead) break;
    }
    __syncthreads();
    // read-out: lane i of the first wave follows entry i of the start node forwards
    const unsigned long long st = s_start;
    int count = 0;
    if (!dead && st >= (unsigned long long)sp.n0 && st < (unsigned long long)sp.n1) {
        count = ecnt[st];
        if (count < 0 || count > n) bad = true, count = 0;
    }
    if (wave == 0 && lane < count) {
        int64_t v = (int64_t)st;
        int r = lane, nw = 0;
        double g = 0.0, cost = DINF;
        bool done = false;
        int32_t *const words = q.out_words + (int64_t)n * sp.l0 + (int64_t)lane * nlev;
        for (int64_t step = 0; step <= nlev; ++step) {          // a path has at most one arc per level
            const int32_t al = earc[v * n + r];
            if (al < 0) {
                cost = g + scaled_end(t, v, frames, reached, lm, bad);
                done = true;
                break;
            }
            const int64_t a = sp.a0 + al;
            if (a < t.out_ptr[v] || a >= t.out_ptr[v + 1] || a >= sp.a1) break;
            const int64_t d = sp.n0 + t.dst[a], ga = t.arc[a];
            if (d < sp.n0 || d >= sp.n1 || ga < 0 || ga >= t.G) break;
            const int32_t ld = t.level[d];
            if (ld <= t.level[v] || ld >= sp.l1) break;
            const int32_t rk = erank[v * n + r];
            if (rk < 0 || rk >= ecnt[d] || ecnt[d] > n) break;
            g = g + arc_cost(lm, sc, t.w[ga], t.lp[a]);
            const int32_t word = t.ol[ga];
            if (word != 0) {
                if (nw >= nlev) break;
                words[nw++] = word;
            }
            v = d, r = rk;
        }
        if (!done) bad = true;
        q.out_cost[(int64_t)b * n + lane] = cost;
        q.out_nwords[(int64_t)b * n + lane] = done ? nw : 0;
    }
    dead = __syncthreads_or(bad) != 0 || dead;
    if (tid == 0) q.out_count[b] = dead ? 0 : count, q.out_status[b] = dead ? 1 : 0;
}

// ---- minimum-Bayes-risk decoding (asr_lattice_mbr_f64) -------------------
// Expected distances alpha' and the arc chain a are int64 at 2^-40, the masses beta', b, gamma int64 at
// 2^-52; every product is llrint(pi * (double)v).  Integer sums commute, so the node sums, the atomic
// adds into beta' and gamma and the wave scans give the same words whatever the schedule.
constexpr int MBR_MAX_WORDS = ASR_LATTICE_MBR_MAX_WORDS;
constexpr int MBR_MAX_COLS = 2 * MBR_MAX_WORDS + 2;     // slots 0 .. S, S = 2 Q + 1
constexpr int64_t MBR_ONE = (int64_t)1 << 40;
constexpr int64_t MBR_SUB = MBR_ONE + 10995116;         // 1 + delta, delta = 1e-5
constexpr int64_t MBR_MASS = (int64_t)1 << 52;
constexpr int64_t MBR_BIG = (int64_t)1 << 60;
constexpr int64_t MBR_EMPTY = -1;

struct MbrArgs {
    Lat t;
    double ac_scale, lm_scale;              // ac_scale NaN: the utterance's own
    const double *arc_cond, *end_cond;      // [A], [N] or NULL: computed here (phase 0)
    const int32_t *init_words, *init_nwords;        // [B][W], [B] or NULL: the tropical best path
    int max_iter, W, C;                     // C = 2 W + 2 columns a node
    int64_t cap;                            // sausage entries an utterance
    int64_t *alpha, *beta;                  // workspace [nodes of the launch][C]
    double *fwd;                            // workspace [nodes of the launch]
    int32_t *out_nwords, *out_words;        // [B], [B][W]
    double *out_conf;                       // [B][W]
    int32_t *out_frames;                    // [B][W]
    double *out_risk;                       // [B]
    int32_t *out_iters, *out_status, *out_count;    // [B]
    int64_t *tab_key, *tab_gamma, *tab_tau; // [B][cap]: (slot << 32 | word), gamma, tau
};

__device__ __forceinline__ int64_t ld64(const int64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void add64(int64_t *p, int64_t v) {
    atomicAdd((unsigned long long *)p, (unsigned long long)v);
}

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int d) { return (int64_t)__shfl_up((long long)v, d); }
__device__ __forceinline__ int64_t shfl_down64(int64_t v, int d) { return (int64_t)__shfl_down((long long)v, d); }
__device__ __forceinline__ int64_t shfl64(int64_t v, int l) { return (int64_t)__shfl((long long)v, l); }

__device__ __forceinline__ int64_t mbr_hash(int64_t key, int64_t cap) {
    const uint64_t h = (uint64_t)key * 0x9E3779B97F4A7C15ull;
    return (int64_t)((h >> 20) % (uint64_t)cap);
}

// gamma(slot, word) += g, tau += tt in the utterance's table; false: the table is full
__device__ __forceinline__ bool mbr_table_add(int64_t *keys, int64_t *gam, int64_t *tau, int64_t cap, int slot,
                                              int32_t word, int64_t g, int64_t tt) {
    const int64_t key = ((int64_t)slot << 32) | (uint32_t)word;
    int64_t i = mbr_hash(key, cap);
    for (int64_t n = 0; n < cap; ++n) {
        const unsigned long long prev = atomicCAS((unsigned long long *)&keys[i], (unsigned long long)MBR_EMPTY,
                                                  (unsigned long long)key);
        if (prev == (unsigned long long)MBR_EMPTY || prev == (unsigned long long)key) {
            add64(&gam[i], g);
            if (tt) add64(&tau[i], tt);
            return true;
        }
        if (++i == cap) i = 0;
    }
    return false;
}

// the table's entry of (slot, word): its index or -1
__device__ __forceinline__ int64_t mbr_table_find(const int64_t *keys, int64_t cap, int slot, int32_t word) {
    const int64_t key = ((int64_t)slot << 32) | (uint32_t)word;
    int64_t i = mbr_hash(key, cap);
    for (int64_t n = 0; n < cap; ++n) {
        const int64_t k = ld64(&keys[i]);
        if (k == key) return i;
        if (k == MBR_EMPTY) return -1;
        if (++i == cap) i = 0;
    }
    return -1;
}

template <int NT>
__global__ __launch_bounds__(NT) void lattice_mbr_kernel(const MbrArgs q) {
    const Lat &t = q.t;
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = t.b_begin + (int)blockIdx.x;
    const int W = q.W, C = q.C;
    __shared__ int64_t s_acc[NW][MBR_MAX_COLS];         // the sums of the node a wave owns
    __shared__ uint8_t s_case[NW][MBR_MAX_COLS];        // the case of every slot of the arc in hand
    __shared__ int32_t s_r[MBR_MAX_COLS];               // the hypothesis in slot form
    __shared__ int64_t s_dc[MBR_MAX_COLS];              // sum of del(r_1 .. r_q)
    __shared__ int64_t s_ae[MBR_MAX_COLS], s_be[MBR_MAX_COLS];  // alpha', beta' of the end node E
    __shared__ int64_t s_gmax[MBR_MAX_COLS];
    __shared__ int32_t s_pick[MBR_MAX_COLS];
    __shared__ int32_t s_words[MBR_MAX_WORDS + 1];
    __shared__ double s_val[NT];
    __shared__ int64_t s_idx[NT];
    __shared__ unsigned long long s_start;
    __shared__ double s_logz;
    __shared__ int s_flags, s_nw, s_go, s_count;
    if (tid == 0) s_start = ~0ull, s_flags = 0, s_nw = 0, s_go = 0, s_count = 0, s_logz = -DINF;
    __syncthreads();
    const Span sp = span_of(t, b);
    if (!sp.ok || !levels_cover(t, sp)) {
        if (tid == 0) {
            q.out_nwords[b] = 0, q.out_risk[b] = DINF, q.out_iters[b] = 0, q.out_count[b] = 0;
            q.out_status[b] = 1;
        }
        return;
    }
    const double sc = scale_of(t, b, q.ac_scale);
    const double lm = q.lm_scale;
    const int frames = t.frames[b], reached = t.reached[b];
    const int64_t nlev = sp.l1 - sp.l0;
    int64_t *const alpha = q.alpha - t.n_begin * C;     // indexed by batch node * C + slot
    int64_t *const beta = q.beta - t.n_begin * C;
    double *const fwd = q.fwd - t.n_begin;
    int64_t *const keys = q.tab_key + (int64_t)b * q.cap;
    int64_t *const gam = q.tab_gamma + (int64_t)b * q.cap;
    int64_t *const tau = q.tab_tau + (int64_t)b * q.cap;
    bool bad = false, dead = false;

    for (int64_t v = sp.n0 + tid; v < sp.n1; v += NT)
        if (t.time[v] == 0 && t.state[v] == t.start) atomicMin(&s_start, (unsigned long long)v);
    __syncthreads();
    const int64_t st = s_start == ~0ull ? -1 : (int64_t)s_start;
    bool none = st < 0;

    // ---- the start hypothesis --------------------------------------------------------------
    if (q.init_words) {
        const int n = q.init_nwords[b];
        if (n < 0 || n > W) {
            if (tid == 0) s_flags = 4;
        } else {
            for (int k = tid; k < n; k += NT) s_words[k] = q.init_words[(int64_t)b * W + k];
            if (tid == 0) s_nw = n;
        }
    } else if (!none) {
        // the tropical best path under the tie rule of asr_lattice_bestpath_f64; cost in fwd, a node's
        // back-pointer in the first word of its own row of beta
        double *const cost = fwd;
        auto bp = [&](int64_t v) -> int32_t & { return *(int32_t *)(beta + v * C); };
        bool nan = false;
        for (int64_t l = sp.l0; l < sp.l1; ++l) {
            const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
            if (!level_range(e0, e1, sp.n0, sp.n1)) {
                bad = true;
            } else {
                for (int64_t e = e0 + tid; e < e1; e += NT) {
                    int64_t v, j0, j1;
                    if (!node_at(t, sp, e, l, v) || !in_arcs_of(t, sp, v, j0, j1)) {
                        bad = true;
                        continue;
                    }
                    const bool is_start = v == st;
                    double c = is_start ? 0.0 : DINF;
                    int64_t best_g = INT64_MAX;
                    int32_t back = -1;
                    for (int64_t j = j0; j < j1; ++j) {
                        int64_t a, u, g;
                        if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
                            bad = true;
                            break;
                        }
                        const double cand = cost[u] + arc_cost(lm, sc, t.w[g], t.lp[a]);
                        if (cand != cand) {
                            nan = true;
                        } else if (cand < c) {
                            c = cand, best_g = g, back = (int32_t)(a - sp.a0);
                        } else if (cand == c && cand < DINF && g <= best_g) {
                            best_g = g, back = (int32_t)(a - sp.a0);
                        }
                    }
                    cost[v] = c;
                    bp(v) = is_start ? -1 : back;
                }
            }
            dead = __syncthreads_or(bad) != 0;
            if (dead) break;
        }
        double m = DINF;
        int64_t mi = -1;
        if (!dead) {
            for (int64_t v = sp.n0 + tid; v < sp.n1; v += NT) {
                const double e = end_cost(t, v, frames, reached, bad);
                const double tot = cost[v] + lm * e;
                if (tot != tot)
                    nan = true;
                else if (tot < m)
                    m = tot, mi = v;
            }
        }
        s_val[tid] = m;
        s_idx[tid] = mi;
        if (nan) atomicOr(&s_flags, 8);
        dead = __syncthreads_or(bad) != 0 || dead;
        if (tid == 0 && !dead) {
            m = DINF, mi = -1;
            if (!(s_flags & 8)) {
                for (int i = 0; i < NT; ++i)
                    if (s_idx[i] >= 0 && (s_val[i] < m || (s_val[i] == m && s_idx[i] < mi)))
                        m = s_val[i], mi = s_idx[i];
            }
            int nw = 0, flags = mi < 0 ? 8 : 0;
            int64_t cur = mi;
            for (int64_t step = 0; step <= nlev && mi >= 0; ++step) {   // a path has at most one arc per level
                const int32_t back = bp(cur);
                if (back < 0) break;
                int64_t a, u, g;
                if (!back_arc_at(t, sp, back, cur, a, u, g)) {
                    flags |= 1;
                    break;
                }
                const int32_t word = t.ol[g];
                if (word != 0) {
                    if (nw >= W) {
                        flags |= 4;
                        break;
                    }
                    s_words[nw++] = word;
                }
                cur = u;
            }
            for (int i = 0, j = nw - 1; i < j; ++i, --j) {      // gathered end to start: path order
                const int32_t x = s_words[i];
                s_words[i] = s_words[j];
                s_words[j] = x;
            }
            s_nw = nw;
            s_flags = flags;
        }
    }
    __syncthreads();
    if (s_flags & 1) dead = true;
    if (s_flags & 8) none = true;

    // ---- phase 0: the log-semiring forward pass, when the conditionals are not given ------------
    const bool own = !q.arc_cond || !q.end_cond;
    if (own && !none && !dead && !(s_flags & 4)) {
        for (int64_t l = sp.l0; l < sp.l1; ++l) {
            const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
            if (!level_range(e0, e1, sp.n0, sp.n1)) {
                bad = true;
            } else {
                for (int64_t e = e0 + tid; e < e1; e += NT) {
                    int64_t v, j0, j1;
                    if (!node_at(t, sp, e, l, v) || !in_arcs_of(t, sp, v, j0, j1)) {
                        bad = true;
                        continue;
                    }
                    const bool is_start = v == st;
                    double m = is_start ? 0.0 : -DINF, s = 0.0;
                    for (int pass = 0; pass < 2 && !bad && !is_start; ++pass) {
                        if (pass == 1) {
                            if (m == -DINF) break;
                            s = 0.0;
                        }
                        for (int64_t j = j0; j < j1; ++j) {
                            int64_t a, u, g;
                            if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
                                bad = true;
                                break;
                            }
                            const double term = log_times(fwd[u], arc_cost(lm, sc, t.w[g], t.lp[a]));
                            if (pass == 0)
                                m = term > m ? term : m;
                            else if (term != -DINF)
                                s += exp(term - m);
                        }
                    }
                    fwd[v] = is_start ? 0.0 : lse_value(m, s);
                }
            }
            dead = __syncthreads_or(bad) != 0;
            if (dead) break;
        }
        if (tid == 0 && !dead) {                // log_z by one lane in node order: the same bits for every NT
            double m = -DINF, s = 0.0;
            bool eb = false;
            for (int pass = 0; pass < 2; ++pass) {
                if (pass == 1 && m == -DINF) break;
                for (int64_t v = sp.n0; v < sp.n1; ++v) {
                    const double en = end_cost(t, v, frames, reached, eb);
                    const double f = fwd[v];
                    if (!(en < DINF) || !(f > -DINF)) continue;
                    const double term = f - lm * en;
                    if (pass == 0)
                        m = term > m ? term : m;
                    else if (term > -DINF)
                        s += exp(term - m);
                }
            }
            s_logz = lse_value(m, s);
            if (eb) s_flags |= 1;
        }
        __syncthreads();
        if (s_flags & 1) dead = true;
    }
    const double logz = s_logz;
    auto arc_pi = [&](int64_t a, int64_t u, int64_t v, int64_t g) -> double {
        double p;
        if (q.arc_cond) {
            p = q.arc_cond[a];
        } else {
            const double x = arc_cost(lm, sc, t.w[g], t.lp[a]);
            const double fu = fwd[u], fv = fwd[v];
            p = (fu == -DINF || !(x < DINF) || fv == -DINF) ? 0.0 : exp((fu - x) - fv);
        }
        return p > 0.0 ? p : 0.0;
    };
    auto stop_pi = [&](int64_t v) -> double {
        double p = 0.0;
        if (q.end_cond) {
            p = q.end_cond[v];
        } else {
            bool eb = false;
            const double en = end_cost(t, v, frames, reached, eb);
            const double f = fwd[v];
            if (en < DINF && f > -DINF && !eb) p = exp((f - lm * en) - logz);
        }
        return p > 0.0 ? p : 0.0;
    };
    {
        bool any = false;
        if (!none && !dead) {
            if (q.end_cond) {
                for (int64_t v = sp.n0 + tid; v < sp.n1; v += NT) any = any || q.end_cond[v] > 0.0;
            } else {
                any = logz > -DINF;
            }
        }
        if (!__syncthreads_or(any)) none = true;
    }

    // ---- the iterations --------------------------------------------------------------------------
    const int nmax = q.max_iter > 1 ? q.max_iter : 1;
    int iters = 0, S = 1;
    int64_t risk = 0;
    const bool run = !none && !dead && !(s_flags & 4);
    while (run) {
        const int Q = s_nw;
        S = 2 * Q + 1;
        const int R = (S + 1 + 63) >> 6;        // rounds of a wave over the slots 0 .. S
        for (int k = tid; k <= S; k += NT) {
            s_r[k] = (k >= 2 && (k & 1) == 0) ? s_words[k / 2 - 1] : 0;
            s_ae[k] = 0;
            s_be[k] = k == S ? MBR_MASS : 0;
            s_gmax[k] = -1;
            s_pick[k] = INT32_MAX;
        }
        for (int64_t i = tid; i < q.cap; i += NT) keys[i] = MBR_EMPTY, gam[i] = 0, tau[i] = 0;
        for (int64_t v = sp.n0 + wave; v < sp.n1; v += NW)     // a row a wave: the live columns alone
            for (int k = lane; k <= S; k += 64) beta[v * C + k] = 0;
        __syncthreads();
        if (tid == 0) {
            int64_t d = 0;
            s_dc[0] = 0;
            for (int k = 1; k <= S; ++k) d += s_r[k] != 0 ? MBR_ONE : 0, s_dc[k] = d;
        }
        __threadfence();
        __syncthreads();

        // the chain a(q) of one in-arc for the lane's slot of a round, with A1, A2 and a(q - 1);
        // carry: the running minimum of min(A1, A2) - D below this round; alast: a of the slot below it
        auto chain = [&](const int64_t *au, int32_t w, int qq, int64_t &carry, int64_t &alast, int64_t &A1,
                         int64_t &A2, int64_t &aprev) -> int64_t {
            const bool act = qq <= S;
            const int64_t ins = w != 0 ? MBR_SUB : 0;
            A1 = MBR_BIG, A2 = MBR_BIG;
            int64_t dq = 0;
            if (act) {
                dq = s_dc[qq];
                A2 = au[qq] + ins;
                if (qq > 0) A1 = au[qq - 1] + (w == s_r[qq] ? 0 : MBR_SUB);
            }
            int64_t x = act ? (A1 < A2 ? A1 : A2) - dq : MBR_BIG;
            for (int d = 1; d < 64; d <<= 1) {  // min-plus prefix scan: exact in integers
                const int64_t o = shfl_up64(x, d);
                if (lane >= d && o < x) x = o;
            }
            if (carry < x) x = carry;
            const int64_t a = x + dq;
            const int64_t up = shfl_up64(a, 1);
            aprev = lane == 0 ? alast : up;
            carry = shfl64(x, 63);
            alast = shfl64(a, 63);
            return a;
        };
        // alpha'(v, .) += pi a(.) for one in-arc, into the wave's sums
        auto forward_arc = [&](const int64_t *au, int32_t w, double pi, int64_t *acc) {
            int64_t carry = MBR_BIG, alast = 0, A1, A2, aprev;
            for (int r = 0; r < R; ++r) {
                const int qq = lane + 64 * r;
                const int64_t a = chain(au, w, qq, carry, alast, A1, A2, aprev);
                if (qq <= S) acc[qq] += llrint(pi * (double)a);
            }
        };
        // one in-arc backwards: the cases of every slot, then b(.) downwards as a segmented suffix sum
        // over the lanes (a slot passes its b on to the slot below exactly when it is case 3), then the
        // adds into beta'(u, .), gamma and tau.  bu NULL: the start node, every slot case 3.
        auto backward_arc = [&](const int64_t *au, int64_t *bu, const int64_t *bv, int32_t w, double pi, int tv) {
            if (bu) {
                int64_t carry = MBR_BIG, alast = 0, A1, A2, aprev;
                for (int r = 0; r < R; ++r) {
                    const int qq = lane + 64 * r;
                    chain(au, w, qq, carry, alast, A1, A2, aprev);
                    uint8_t cs = 0;
                    if (qq >= 1 && qq <= S) {
                        const int64_t A3 = aprev + (s_r[qq] != 0 ? MBR_ONE : 0);
                        cs = (A1 <= A2 && A1 <= A3) ? 1 : (A2 <= A3 ? 2 : 3);
                    }
                    s_case[wave][qq] = cs;
                }
            } else {
                for (int r = 0; r < R; ++r) {
                    const int qq = lane + 64 * r;
                    s_case[wave][qq] = (qq >= 1 && qq <= S) ? 3 : 0;
                }
            }
            __builtin_amdgcn_wave_barrier();
            int64_t carry = 0;
            for (int r = R - 1; r >= 0; --r) {
                const int qq = lane + 64 * r;
                const bool act = qq <= S;
                int64_t v = act ? llrint(pi * (double)ld64(&bv[qq])) : 0;
                int f = (act && qq + 1 <= S && s_case[wave][qq + 1] == 3) ? 1 : 0;
                for (int d = 1; d < 64; d <<= 1) {
                    const int64_t vo = shfl_down64(v, d);
                    const int fo = __shfl_down(f, d);
                    if (lane + d < 64 && f) v += vo, f = fo;
                }
                if (f) v += carry;
                carry = shfl64(v, 0);
                if (!act || v <= 0) continue;
                const int cs = s_case[wave][qq];
                bool ok = true;
                if (qq == 0) {
                    if (bu) add64(&bu[0], v);
                } else if (cs == 1) {
                    add64(&bu[qq - 1], v);
                    ok = mbr_table_add(keys, gam, tau, q.cap, qq, w, v, (v >> 12) * (int64_t)tv);
                } else if (cs == 2) {
                    add64(&bu[qq], v);
                } else {
                    ok = mbr_table_add(keys, gam, tau, q.cap, qq, 0, v, 0);
                }
                if (!ok) atomicOr(&s_flags, 2);
            }
            __builtin_amdgcn_wave_barrier();
        };

        // forward, levels upwards: a wave owns a node and takes its in-arcs in turn
        for (int64_t l = sp.l0; l < sp.l1; ++l) {
            const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
            if (!level_range(e0, e1, sp.n0, sp.n1)) {
                bad = true;
            } else {
                for (int64_t e = e0 + wave; e < e1; e += NW) {
                    int64_t v, j0, j1;
                    if (!node_at(t, sp, e, l, v) || !in_arcs_of(t, sp, v, j0, j1)) {
                        bad = true;
                        continue;
                    }
                    int64_t *const av = alpha + v * C;
                    if (v == st) {
                        for (int k = lane; k <= S; k += 64) av[k] = s_dc[k];
                        continue;
                    }
                    int64_t *const acc = s_acc[wave];
                    for (int k = lane; k <= S; k += 64) acc[k] = 0;
                    for (int64_t j = j0; j < j1; ++j) {
                        int64_t a, u, g;
                        if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
                            bad = true;
                            break;
                        }
                        const double pi = arc_pi(a, u, v, g);
                        if (pi > 0.0) forward_arc(alpha + u * C, t.ol[g], pi, acc);
                    }
                    for (int k = lane; k <= S; k += 64) av[k] = acc[k];
                }
            }
            dead = __syncthreads_or(bad) != 0;  // also makes the level's alpha' visible to every wave
            if (dead) break;
        }
        if (dead) break;
        // the end node E: a stop arc from every node that can end a path, the nodes dealt to the waves;
        // the waves' sums meet in s_ae (integers: any order)
        {
            int64_t *const acc = s_acc[wave];
            for (int k = lane; k <= S; k += 64) acc[k] = 0;
            for (int64_t v = sp.n0 + wave; v < sp.n1; v += NW) {
                const double pi = stop_pi(v);
                if (pi > 0.0) forward_arc(alpha + v * C, 0, pi, acc);
            }
        }
        __syncthreads();
        for (int k = tid; k <= S; k += NT) {
            int64_t sum = 0;
            for (int w = 0; w < NW; ++w) sum += s_acc[w][k];
            s_ae[k] = sum;
        }
        for (int64_t v = sp.n0 + wave; v < sp.n1; v += NW) {
            const double pi = stop_pi(v);
            if (pi > 0.0) backward_arc(alpha + v * C, beta + v * C, s_be, 0, pi, frames);
        }
        __threadfence();
        __syncthreads();
        risk = s_ae[S];
        // backward, levels downwards
        for (int64_t l = sp.l1 - 1; l >= sp.l0; --l) {
            const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];     // checked in the forward
            for (int64_t e = e0 + wave; e < e1; e += NW) {
                int64_t v, j0, j1;
                if (!node_at(t, sp, e, l, v) || !in_arcs_of(t, sp, v, j0, j1)) {
                    bad = true;
                    continue;
                }
                if (v == st) {
                    backward_arc(nullptr, nullptr, beta + v * C, 0, 1.0, 0);
                    continue;
                }
                const int tv = t.time[v];
                for (int64_t j = j0; j < j1; ++j) {
                    int64_t a, u, g;
                    if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
                        bad = true;
                        break;
                    }
                    const double pi = arc_pi(a, u, v, g);
                    if (pi > 0.0) backward_arc(alpha + u * C, beta + u * C, beta + v * C, t.ol[g], pi, tv);
                }
            }
            __threadfence();
            dead = __syncthreads_or(bad) != 0;
            if (dead) break;
        }
        if (dead) break;
        ++iters;
        if (s_flags & 2) break;                 // the sausage buffer is full: the caller redoes the utterance
        if (iters >= nmax) break;
        // update: every slot takes the word of the largest gamma; ties: its own word, else the smallest
        for (int64_t i = tid; i < q.cap; i += NT) {
            const int64_t k = ld64(&keys[i]);
            if (k < 0) continue;
            const int slot = (int)(k >> 32);
            const int64_t g = ld64(&gam[i]);
            if (slot >= 1 && slot <= S && g > 0) atomicMax((long long *)&s_gmax[slot], (long long)g);
        }
        __syncthreads();
        for (int64_t i = tid; i < q.cap; i += NT) {
            const int64_t k = ld64(&keys[i]);
            if (k < 0) continue;
            const int slot = (int)(k >> 32);
            const int32_t word = (int32_t)(k & 0xFFFFFFFFll);
            if (slot >= 1 && slot <= S && ld64(&gam[i]) == s_gmax[slot])
                atomicMin(&s_pick[slot], word == s_r[slot] ? -1 : word);
        }
        __syncthreads();
        if (tid == 0) {
            int n = 0, changed = 0, flags = 0;
            for (int k = 1; k <= S; ++k) {
                const int32_t pick = s_pick[k];
                const int32_t word = pick == INT32_MAX ? 0 : (pick == -1 ? s_r[k] : pick);
                if (word == 0) continue;
                if (n >= W) {
                    flags = 4;                  // the hypothesis outgrew the device's columns
                    break;
                }
                if (n >= Q || s_words[n] != word) changed = 1;
                s_words[n++] = word;
            }
            if (n != Q) changed = 1;
            s_nw = n;
            s_go = changed && !flags;
            if (flags) s_flags |= flags;
        }
        __syncthreads();
        const int go = s_go;
        __syncthreads();
        if (!go) break;
    }

    // ---- the result: of the last evaluated hypothesis ---------------------------------------------
    dead = __syncthreads_or(bad) != 0 || dead;
    const int flags = s_flags & 6;
    const bool have = run && !dead && !flags;
    const int Q = have ? (S - 1) / 2 : 0;
    if (have) {
        for (int k = tid; k < Q; k += NT) {
            const int32_t word = s_r[2 * k + 2];
            const int64_t i = mbr_table_find(keys, q.cap, 2 * k + 2, word);
            const int64_t g = i >= 0 ? ld64(&gam[i]) : 0, tt = i >= 0 ? ld64(&tau[i]) : 0;
            const int64_t g12 = g >> 12;
            q.out_words[(int64_t)b * W + k] = word;
            q.out_conf[(int64_t)b * W + k] = (double)g / (double)MBR_MASS;
            q.out_frames[(int64_t)b * W + k] = g12 > 0 ? (int32_t)llrint((double)tt / (double)g12) : 0;
        }
        int n = 0;
        for (int64_t i = tid; i < q.cap; i += NT) n += (ld64(&keys[i]) >= 0 && ld64(&gam[i]) > 0) ? 1 : 0;
        if (n) atomicAdd(&s_count, n);
    }
    __syncthreads();
    if (tid == 0) {
        q.out_nwords[b] = Q;
        q.out_risk[b] = have ? (double)risk / (double)MBR_ONE : DINF;
        q.out_iters[b] = have ? iters : 0;
        q.out_count[b] = have ? s_count : 0;
        q.out_status[b] = (dead ? 1 : 0) | (dead ? 0 : flags);
    }
}

}  // namespace

extern "C" int asr_lattice_bestpath_supported(int64_t N, int64_t A, int64_t L) { return sizes_ok(N, A, L) ? 1 : 0; }

extern "C" int64_t asr_lattice_bestpath_workspace_bytes(int64_t num_nodes, int num_pairs) {
    if (num_nodes < 0 || num_pairs < 1 || !sizes_ok(num_nodes, 0, 0)) return 0;
    return up16(num_nodes * num_pairs * 8) + up16(num_nodes * num_pairs * 4) + 16;
}

extern "C" int asr_lattice_posterior_supported(int64_t N, int64_t A, int64_t L) { return sizes_ok(N, A, L) ? 1 : 0; }

extern "C" int64_t asr_lattice_posterior_workspace_bytes(int64_t num_nodes) {
    if (num_nodes < 0 || !sizes_ok(num_nodes, 0, 0)) return 0;
    return 2 * up16(num_nodes * 8) + 16;
}

extern "C" int asr_lattice_bestpath_f64(
    int B, int b_begin, int b_count, int num_pairs, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    const double *acoustic_scales, const double *lm_scales, int64_t num_states, int64_t num_graph_arcs,
    const float *arc_weight, const int32_t *arc_olabel, const float *final_cost, int start, int threads,
    double *out_cost, int32_t *out_num_words, int32_t *out_words, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream) {
    BestArgs q;
    const int rc = fill_lat(q.t, LAT_LP | LAT_OLABEL, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off,
                            node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc,
                            lat_lp, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final,
                            own_scale, num_states, num_graph_arcs, arc_weight, arc_olabel, nullptr, final_cost, start);
    if (rc != ASR_OK) return rc;
    if (num_pairs < 0 || !threads_ok(threads)) return ASR_EINVAL;
    if (b_count == 0 || num_pairs == 0) return ASR_OK;
    if (!acoustic_scales || !lm_scales || !out_cost || !out_num_words || !out_status || (L > 0 && !out_words))
        return ASR_EINVAL;
    const int64_t n = h_node_off[b_begin + b_count] - h_node_off[b_begin];
    if ((int64_t)b_count * num_pairs >= ((int64_t)1 << 31)) return ASR_EUNSUPPORTED;
    const int64_t need = asr_lattice_bestpath_workspace_bytes(n, num_pairs);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    q.P = num_pairs;
    q.ac_scale = acoustic_scales;
    q.lm_scale = lm_scales;
    q.cost = (double *)workspace;
    q.bp = (int32_t *)((uint8_t *)workspace + up16(n * num_pairs * 8));
    q.n_launch = n;
    q.out_cost = out_cost;
    q.out_nwords = out_num_words;
    q.out_words = out_words;
    q.out_status = out_status;
    return launch_by_threads(threads, 64, (int64_t)b_count * num_pairs, stream, q, lattice_bestpath_kernel<64>,
                             lattice_bestpath_kernel<128>, lattice_bestpath_kernel<256>);
}

extern "C" int asr_lattice_posterior_f64(
    int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, double *out_log_z,
    double *out_arc_log_post, double *out_node_log_post, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream) {
    PostArgs q;
    const int rc = fill_lat(q.t, LAT_LP | LAT_OLABEL, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off,
                            node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc,
                            lat_lp, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final,
                            own_scale, num_states, num_graph_arcs, arc_weight, arc_olabel, nullptr, final_cost, start);
    if (rc != ASR_OK) return rc;
    if (!threads_ok(threads)) return ASR_EINVAL;
    if (b_count == 0) return ASR_OK;
    if (!out_log_z || !out_status || (A > 0 && !out_arc_log_post) || (N > 0 && !out_node_log_post)) return ASR_EINVAL;
    const int64_t n = h_node_off[b_begin + b_count] - h_node_off[b_begin];
    const int64_t need = asr_lattice_posterior_workspace_bytes(n);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    q.ac_scale = acoustic_scale;
    q.lm_scale = lm_scale;
    q.fwd = (double *)workspace;
    q.bwd = (double *)((uint8_t *)workspace + up16(n * 8));
    q.log_z = out_log_z;
    q.arc_post = out_arc_log_post;
    q.node_post = out_node_log_post;
    q.out_status = out_status;
    return launch_by_threads(threads, 64, b_count, stream, q, lattice_posterior_kernel<64>,
                             lattice_posterior_kernel<128>, lattice_posterior_kernel<256>);
}

extern "C" int asr_lattice_nbest_supported(int64_t N, int64_t A, int64_t L, int n) {
    return sizes_ok(N, A, L) && n >= 1 && n <= NBEST_MAX ? 1 : 0;
}

extern "C" int64_t asr_lattice_nbest_workspace_bytes(int64_t num_nodes, int n) {
    if (num_nodes < 0 || n < 1 || n > NBEST_MAX || !sizes_ok(num_nodes, 0, 0)) return 0;
    const int64_t e = num_nodes * n;
    return 2 * up16(e * 8) + 3 * up16(e * 4) + up16(num_nodes * 4) + 16;
}

extern "C" int asr_lattice_nbest_f64(
    int B, int b_begin, int b_count, int n, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, int32_t *out_count,
    double *out_cost, int32_t *out_num_words, int32_t *out_words, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream) {
    NbestArgs q;
    const int rc = fill_lat(q.t, LAT_LP | LAT_OLABEL, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off,
                            node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc,
                            lat_lp, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final,
                            own_scale, num_states, num_graph_arcs, arc_weight, arc_olabel, nullptr, final_cost, start);
    if (rc != ASR_OK) return rc;
    if (n < 1 || !threads_ok(threads)) return ASR_EINVAL;
    if (n > NBEST_MAX) return ASR_EUNSUPPORTED;
    if (b_count == 0) return ASR_OK;
    if (!out_count || !out_cost || !out_num_words || !out_status || (L > 0 && !out_words)) return ASR_EINVAL;
    const int64_t nodes = h_node_off[b_begin + b_count] - h_node_off[b_begin];
    const int64_t need = asr_lattice_nbest_workspace_bytes(nodes, n);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    const int64_t e = nodes * n;
    uint8_t *p = (uint8_t *)workspace;
    q.n = n;
    q.ac_scale = acoustic_scale;
    q.lm_scale = lm_scale;
    q.ec = (double *)p, p += up16(e * 8);
    q.eh = (uint64_t *)p, p += up16(e * 8);
    q.elen = (int32_t *)p, p += up16(e * 4);
    q.earc = (int32_t *)p, p += up16(e * 4);
    q.erank = (int32_t *)p, p += up16(e * 4);
    q.ecnt = (int32_t *)p;
    q.out_count = out_count;
    q.out_cost = out_cost;
    q.out_nwords = out_num_words;
    q.out_words = out_words;
    q.out_status = out_status;
    // threads 0: four waves, four nodes of a level at a time (section 4.22)
    return launch_by_threads(threads, 256, b_count, stream, q, lattice_nbest_kernel<64>, lattice_nbest_kernel<128>,
                             lattice_nbest_kernel<256>);
}

extern "C" int asr_lattice_mbr_supported(int64_t N, int64_t A, int64_t L, int max_words) {
    return sizes_ok(N, A, L) && max_words >= 1 && max_words <= MBR_MAX_WORDS ? 1 : 0;
}

extern "C" int64_t asr_lattice_mbr_workspace_bytes(int64_t num_nodes, int max_words) {
    if (num_nodes < 0 || max_words < 1 || max_words > MBR_MAX_WORDS || !sizes_ok(num_nodes, 0, 0)) return 0;
    const int64_t cols = 2 * (int64_t)max_words + 2;
    return 2 * up16(num_nodes * cols * 8) + up16(num_nodes * 8) + 16;
}

extern "C" int asr_lattice_mbr_f64(
    int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, const double *arc_cond,
    const double *end_cond, const int32_t *init_words, const int32_t *init_num_words, int max_iterations,
    int max_words, int64_t sausage_cap, int32_t *out_num_words, int32_t *out_words, double *out_confidence,
    int32_t *out_frames, double *out_risk, int32_t *out_iterations, int32_t *out_status,
    int32_t *out_sausage_count, int64_t *out_sausage_key, int64_t *out_sausage_gamma, int64_t *out_sausage_tau,
    void *workspace, int64_t workspace_bytes, void *stream) {
    MbrArgs q;
    const int rc = fill_lat(q.t, LAT_LP | LAT_OLABEL, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off,
                            node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc,
                            lat_lp, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final,
                            own_scale, num_states, num_graph_arcs, arc_weight, arc_olabel, nullptr, final_cost, start);
    if (rc != ASR_OK) return rc;
    if (max_words < 1 || max_iterations < 0 || sausage_cap < 1 || !threads_ok(threads)) return ASR_EINVAL;
    if (max_words > MBR_MAX_WORDS || sausage_cap >= ((int64_t)1 << 31)) return ASR_EUNSUPPORTED;
    if ((init_words == nullptr) != (init_num_words == nullptr)) return ASR_EINVAL;
    if (b_count == 0) return ASR_OK;
    if (!out_num_words || !out_words || !out_confidence || !out_frames || !out_risk || !out_iterations ||
        !out_status || !out_sausage_count || !out_sausage_key || !out_sausage_gamma || !out_sausage_tau)
        return ASR_EINVAL;
    const int64_t n = h_node_off[b_begin + b_count] - h_node_off[b_begin];
    const int64_t need = asr_lattice_mbr_workspace_bytes(n, max_words);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    const int64_t cols = 2 * (int64_t)max_words + 2;
    uint8_t *p = (uint8_t *)workspace;
    q.ac_scale = acoustic_scale;
    q.lm_scale = lm_scale;
    q.arc_cond = arc_cond;
    q.end_cond = end_cond;
    q.init_words = init_words;
    q.init_nwords = init_num_words;
    q.max_iter = max_iterations;
    q.W = max_words;
    q.C = (int)cols;
    q.cap = sausage_cap;
    q.alpha = (int64_t *)p, p += up16(n * cols * 8);
    q.beta = (int64_t *)p, p += up16(n * cols * 8);
    q.fwd = (double *)p;
    q.out_nwords = out_num_words;
    q.out_words = out_words;
    q.out_conf = out_confidence;
    q.out_frames = out_frames;
    q.out_risk = out_risk;
    q.out_iters = out_iterations;
    q.out_status = out_status;
    q.out_count = out_sausage_count;
    q.tab_key = out_sausage_key;
    q.tab_gamma = out_sausage_gamma;
    q.tab_tau = out_sausage_tau;
    // threads 0: four waves, four nodes of a level at a time
    return launch_by_threads(threads, 256, b_count, stream, q, lattice_mbr_kernel<64>, lattice_mbr_kernel<128>,
                             lattice_mbr_kernel<256>);
}
