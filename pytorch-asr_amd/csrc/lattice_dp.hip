// Dynamic programmes over a batch of pruned lattices that stays on the device (include/asr_amd.h:
// asr_lattice_bestpath_f64, asr_lattice_posterior_f64, asr_lattice_nbest_f64 and their _supported /
// _workspace_bytes).
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
//
// All synchronise with workgroup barriers only.  Every node, arc, level and graph index read from
// memory is range-checked before it is used (the tensors may come from a caller): a violation raises
// the utterance's status word and ends its workgroup.  Every loop is bounded by the counts passed in.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

constexpr double DINF = __builtin_huge_val();

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct Lat {
    int B;
    int64_t N, A, L, G, S;                  // nodes, arcs, levels of the batch; graph arcs and states
    const int64_t *node_off, *arc_off, *level_off;      // [B + 1]
    const int32_t *time, *state, *level;    // [N]; level: index into level_ptr
    const int32_t *src, *dst;               // [A] node indices of the utterance
    const int64_t *arc;                     // [A] arc index in the graph
    const float *lp;                        // [A]
    const int32_t *level_ptr, *level_node;  // [L + 1], [N]: the nodes of a level (batch indices)
    const int32_t *in_ptr, *in_arc;         // [N + 1], [A]: the in-arcs of a node (batch indices)
    const int32_t *out_ptr;                 // [N + 1]: the out-arcs of node v are [out_ptr[v], out_ptr[v + 1])
    const int32_t *frames, *reached;        // [B]
    const double *own_scale;                // [B] the scale of the search
    const float *w, *fin;                   // graph: [G], [S]
    const int32_t *ol;                      // [G]
    int start;
    int b_begin, b_count;
    int64_t n_begin;                        // node_off[b_begin]: the workspace starts there
};

struct Span {
    int64_t n0, n1, a0, a1, l0, l1;
    bool ok;
};

__device__ __forceinline__ Span span_of(const Lat &t, int b) {
    Span s;
    s.n0 = t.node_off[b], s.n1 = t.node_off[b + 1];
    s.a0 = t.arc_off[b], s.a1 = t.arc_off[b + 1];
    s.l0 = t.level_off[b], s.l1 = t.level_off[b + 1];
    s.ok = t.n_begin <= s.n0 && s.n0 <= s.n1 && s.n1 <= t.N && 0 <= s.a0 && s.a0 <= s.a1 && s.a1 <= t.A &&
           0 <= s.l0 && s.l0 <= s.l1 && s.l1 <= t.L;
    return s;
}

// x = fl(fl(lm w) - fl(sc lp)); this file is compiled with -ffp-contract=off
__device__ __forceinline__ double arc_cost(double lm, double sc, float w, float lp) {
    const double a = lm * (double)w;
    const double b = sc * (double)lp;
    return a - b;
}

// the unscaled cost of stopping at node v (+inf: not an end node)
__device__ __forceinline__ double end_cost(const Lat &t, int64_t v, int frames, int reached, bool &bad) {
    if (t.time[v] != frames) return DINF;
    if (!reached) return 0.0;
    const int s = t.state[v];
    if (s < 0 || s >= t.S) {
        bad = true;
        return DINF;
    }
    return (double)t.fin[s];
}

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
    bool fail = !sp.ok;
    if (!fail) {
        const int32_t p0 = t.level_ptr[sp.l0], p1 = t.level_ptr[sp.l1];
        fail = p0 != sp.n0 || p1 != sp.n1;      // the utterance's levels hold exactly its nodes
    }
    if (fail) {                                  // uniform: every lane read the same words
        if (tid == 0) {
            q.out_cost[3 * o] = q.out_cost[3 * o + 1] = q.out_cost[3 * o + 2] = DINF;
            q.out_nwords[o] = 0;
            q.out_status[o] = 1;
        }
        return;
    }
    double sc = q.ac_scale[pr];
    if (sc != sc) sc = t.own_scale[b];
    const double lm = q.lm_scale[pr];
    double *const cost = q.cost + (int64_t)pr * q.n_launch - t.n_begin;        // indexed by batch node
    int32_t *const bp = q.bp + (int64_t)pr * q.n_launch - t.n_begin;
    bool bad = false, nan = false, dead = false;
    for (int64_t l = sp.l0; l < sp.l1; ++l) {
        const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
        if (e0 < sp.n0 || e0 > e1 || e1 > sp.n1) {
            bad = true;
        } else {
            for (int64_t e = e0 + tid; e < e1; e += NT) {
                const int64_t v = t.level_node[e];
                if (v < sp.n0 || v >= sp.n1 || t.level[v] != l) {
                    bad = true;
                    continue;
                }
                const bool is_start = t.time[v] == 0 && t.state[v] == t.start;
                double c = is_start ? 0.0 : DINF;
                int64_t best_g = INT64_MAX;
                int32_t back = -1;
                const int64_t j0 = t.in_ptr[v], j1 = t.in_ptr[v + 1];
                if (j0 < sp.a0 || j0 > j1 || j1 > sp.a1) {
                    bad = true;
                    continue;
                }
                for (int64_t j = j0; j < j1; ++j) {
                    const int64_t a = t.in_arc[j];
                    if (a < sp.a0 || a >= sp.a1) {
                        bad = true;
                        break;
                    }
                    const int64_t u = sp.n0 + t.src[a], g = t.arc[a];
                    if (sp.n0 + t.dst[a] != v || u < sp.n0 || u >= sp.n1 || g < 0 || g >= t.G) {
                        bad = true;
                        break;
                    }
                    const int32_t lu = t.level[u];
                    if (lu < sp.l0 || lu >= l) {           // the level must rise: cost[u] is final
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
            const int64_t a = sp.a0 + back;
            if (a >= sp.a1) {
                bad = true;
                break;
            }
            const int64_t g = t.arc[a], u = sp.n0 + t.src[a];
            if (g < 0 || g >= t.G || u < sp.n0 || u >= sp.n1 || t.level[u] >= t.level[cur]) {
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

__device__ __forceinline__ double lse_value(double m, double s) { return m == -DINF ? -DINF : m + log(s); }

// a - x for log weights: -inf as soon as the path weight is zero
__device__ __forceinline__ double log_times(double a, double x) { return (a == -DINF || x == DINF) ? -DINF : a - x; }

template <int NT>
__global__ __launch_bounds__(NT) void lattice_posterior_kernel(const PostArgs q) {
    const Lat &t = q.t;
    const int tid = threadIdx.x;
    const int b = t.b_begin + (int)blockIdx.x;
    __shared__ int64_t s_start;
    if (tid == 0) s_start = INT64_MAX;
    __syncthreads();
    const Span sp = span_of(t, b);
    bool fail = !sp.ok;
    if (!fail) fail = t.level_ptr[sp.l0] != sp.n0 || t.level_ptr[sp.l1] != sp.n1;
    if (fail) {
        if (tid == 0) q.log_z[b] = -DINF, q.out_status[b] = 1;
        return;
    }
    double sc = q.ac_scale;
    if (sc != sc) sc = t.own_scale[b];
    const double lm = q.lm_scale;
    double *const fwd = q.fwd - t.n_begin, *const bwd = q.bwd - t.n_begin;
    const int frames = t.frames[b], reached = t.reached[b];
    bool bad = false, dead = false;
    // forward, levels upwards
    for (int64_t l = sp.l0; l < sp.l1; ++l) {
        const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
        if (e0 < sp.n0 || e0 > e1 || e1 > sp.n1) {
            bad = true;
        } else {
            for (int64_t e = e0 + tid; e < e1; e += NT) {
                const int64_t v = t.level_node[e];
                if (v < sp.n0 || v >= sp.n1 || t.level[v] != l) {
                    bad = true;
                    continue;
                }
                const bool is_start = t.time[v] == 0 && t.state[v] == t.start;
                if (is_start) atomicMin((unsigned long long *)&s_start, (unsigned long long)v);
                const int64_t j0 = t.in_ptr[v], j1 = t.in_ptr[v + 1];
                if (j0 < sp.a0 || j0 > j1 || j1 > sp.a1) {
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
                        const int64_t a = t.in_arc[j];
                        if (a < sp.a0 || a >= sp.a1) {
                            bad = true;
                            break;
                        }
                        const int64_t u = sp.n0 + t.src[a], g = t.arc[a];
                        if (sp.n0 + t.dst[a] != v || u < sp.n0 || u >= sp.n1 || g < 0 || g >= t.G) {
                            bad = true;
                            break;
                        }
                        const int32_t lu = t.level[u];
                        if (lu < sp.l0 || lu >= l) {
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
                const double en = end_cost(t, v, frames, reached, bad);
                const double stop = en < DINF ? 0.0 - lm * en : -DINF;
                const int64_t j0 = t.out_ptr[v], j1 = t.out_ptr[v + 1];
                if (j0 < sp.a0 || j0 > j1 || j1 > sp.a1) {
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
                        const int64_t d = sp.n0 + t.dst[a], g = t.arc[a];
                        if (sp.n0 + t.src[a] != v || d < sp.n0 || d >= sp.n1 || g < 0 || g >= t.G) {
                            bad = true;
                            break;
                        }
                        const int32_t ld = t.level[d];
                        if (ld <= l || ld >= sp.l1) {
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
            const int64_t u = sp.n0 + t.src[a], d = sp.n0 + t.dst[a], g = t.arc[a];
            if (u < sp.n0 || u >= sp.n1 || d < sp.n0 || d >= sp.n1 || g < 0 || g >= t.G) {
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

// fl(lm end(v)) as Lattice._end_costs has it: 0 at the last time of a partial lattice
__device__ __forceinline__ double scaled_end(const Lat &t, int64_t v, int frames, int reached, double lm, bool &bad) {
    if (t.time[v] != frames) return DINF;
    if (!reached) return 0.0;
    const int s = t.state[v];
    if (s < 0 || s >= t.S) {
        bad = true;
        return DINF;
    }
    return lm * (double)t.fin[s];
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
    bool fail = !sp.ok;
    if (!fail) fail = t.level_ptr[sp.l0] != sp.n0 || t.level_ptr[sp.l1] != sp.n1;
    if (fail) {
        if (tid == 0) q.out_count[b] = 0, q.out_status[b] = 1;
        return;
    }
    double sc = q.ac_scale;
    if (sc != sc) sc = t.own_scale[b];
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
        if (e0 < sp.n0 || e0 > e1 || e1 > sp.n1) {
            bad = true;
        } else {
            for (int64_t e = e0 + wave; e < e1; e += NW) {      // everything here is uniform in the wave
                const int64_t v = t.level_node[e];
                if (v < sp.n0 || v >= sp.n1 || t.level[v] != l) {
                    bad = true;
                    continue;
                }
                if (lane == 0 && t.time[v] == 0 && t.state[v] == t.start) atomicMin(&s_start, (unsigned long long)v);
                const int64_t j0 = t.out_ptr[v], j1 = t.out_ptr[v + 1];
                if (j0 < sp.a0 || j0 > j1 || j1 > sp.a1) {
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
                        const int64_t d = sp.n0 + t.dst[a], g = t.arc[a];
                        if (sp.n0 + t.src[a] != v || d < sp.n0 || d >= sp.n1 || g < 0 || g >= t.G) {
                            bad = true, has = false;
                        } else {
                            const int32_t ld = t.level[d];
                            if (ld <= l || ld >= sp.l1) {       // the level must rise: list(d) is final
                                bad = true, has = false;
                            } else {
                                x = arc_cost(lm, sc, t.w[g], t.lp[a]);
                                olab = t.ol[g];
                                dcnt = ecnt[d];
                                dbase = d * n;
                                if (dcnt < 0 || dcnt > n) bad = true, has = false;
                                if (!(x < DINF)) has = false;   // +inf or NaN: no candidate survives
                            }
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

bool sizes_ok(int64_t N, int64_t A, int64_t L) {
    const int64_t lim = ((int64_t)1 << 31) - 1;
    return N >= 0 && A >= 0 && L >= 0 && N < lim && A < lim && L < lim;
}

// the host copies of the offsets: [B + 1], from 0 to total, never decreasing
bool offsets_ok(const int64_t *h, int B, int64_t total) {
    if (!h || h[0] != 0 || h[B] != total) return false;
    for (int b = 0; b < B; ++b)
        if (h[b + 1] < h[b]) return false;
    return true;
}

int fill(Lat &t, int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
         const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
         const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
         const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
         const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
         const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
         int64_t S, int64_t G, const float *arc_weight, const int32_t *arc_olabel, const float *final_cost,
         int start) {
    if (B < 0 || b_begin < 0 || b_count < 0 || (int64_t)b_begin + b_count > B) return ASR_EINVAL;
    if (N < 0 || A < 0 || L < 0 || S < 1 || G < 0 || start < 0 || start >= S) return ASR_EINVAL;
    if (!sizes_ok(N, A, L)) return ASR_EUNSUPPORTED;
    if (!offsets_ok(h_node_off, B, N) || !offsets_ok(h_arc_off, B, A) || !offsets_ok(h_level_off, B, L))
        return ASR_EINVAL;
    for (int b = 0; b < B; ++b) {               // a level holds a node; arcs need two nodes on two levels
        const int64_t n = h_node_off[b + 1] - h_node_off[b], l = h_level_off[b + 1] - h_level_off[b];
        if (l > n || (n > 0 && l < 1) || (h_arc_off[b + 1] > h_arc_off[b] && l < 2)) return ASR_EINVAL;
    }
    if (!node_off || !arc_off || !level_off || !level_ptr || !in_ptr || !out_ptr || !num_frames || !reached_final ||
        !own_scale || !final_cost)
        return ASR_EINVAL;
    if (N > 0 && (!node_time || !node_state || !node_level || !level_node)) return ASR_EINVAL;
    if (A > 0 && (!lat_src || !lat_dst || !lat_arc || !lat_lp || !in_arc || !arc_weight || !arc_olabel))
        return ASR_EINVAL;
    t = Lat{B, N, A, L, G, S, node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst,
            lat_arc, lat_lp, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final, own_scale,
            arc_weight, final_cost, arc_olabel, start, b_begin, b_count, h_node_off[b_begin]};
    return ASR_OK;
}

bool threads_ok(int threads) { return threads == 0 || threads == 64 || threads == 128 || threads == 256; }

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
    const int rc = fill(q.t, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off, node_off, arc_off,
                        level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc, lat_lp, level_ptr,
                        level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final, own_scale, num_states,
                        num_graph_arcs, arc_weight, arc_olabel, final_cost, start);
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
    const dim3 grid((unsigned)((int64_t)b_count * num_pairs));
    switch (threads) {
    case 256: hipLaunchKernelGGL(lattice_bestpath_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, q); break;
    case 128: hipLaunchKernelGGL(lattice_bestpath_kernel<128>, grid, dim3(128), 0, (hipStream_t)stream, q); break;
    default: hipLaunchKernelGGL(lattice_bestpath_kernel<64>, grid, dim3(64), 0, (hipStream_t)stream, q); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
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
    const int rc = fill(q.t, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off, node_off, arc_off,
                        level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc, lat_lp, level_ptr,
                        level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final, own_scale, num_states,
                        num_graph_arcs, arc_weight, arc_olabel, final_cost, start);
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
    const dim3 grid((unsigned)b_count);
    switch (threads) {
    case 256: hipLaunchKernelGGL(lattice_posterior_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, q); break;
    case 128: hipLaunchKernelGGL(lattice_posterior_kernel<128>, grid, dim3(128), 0, (hipStream_t)stream, q); break;
    default: hipLaunchKernelGGL(lattice_posterior_kernel<64>, grid, dim3(64), 0, (hipStream_t)stream, q); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
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
    const int rc = fill(q.t, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off, node_off, arc_off,
                        level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc, lat_lp, level_ptr,
                        level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final, own_scale, num_states,
                        num_graph_arcs, arc_weight, arc_olabel, final_cost, start);
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
    const dim3 grid((unsigned)b_count);
    switch (threads) {                          // 0: four waves, four nodes of a level at a time (section 4.22)
    case 64: hipLaunchKernelGGL(lattice_nbest_kernel<64>, grid, dim3(64), 0, (hipStream_t)stream, q); break;
    case 128: hipLaunchKernelGGL(lattice_nbest_kernel<128>, grid, dim3(128), 0, (hipStream_t)stream, q); break;
    default: hipLaunchKernelGGL(lattice_nbest_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, q); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
