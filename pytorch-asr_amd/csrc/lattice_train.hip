// Sequence-discriminative training statistics over a batch of pruned lattices that stays on the device
// (include/asr_amd.h: asr_lattice_seqtrain_f64, asr_lattice_seqtrain_supported,
// asr_lattice_seqtrain_workspace_bytes): the denominator of lattice MMI and
// boosted MMI (log Z and the arc occupancies) and the sMBR objective (the expected frame accuracy and its
// derivative), with the arc scores read from the LIVE log_probs [T, B, C], and the occupancies delivered
// as the [T, B, C] tensor the encoder's backward takes.  LatticeBatch.seq_objective of
// att_speech/wfst_lattice.py is the numpy twin.
//
// The batch is the one of csrc/lattice_dp.hip (nodes by (utterance, time, state), arcs by (utterance,
// source node, graph arc), the (time, epsilon rank) levels, the in-arcs of every node), and the kernel
// has the shape of lattice_posterior_kernel: one workgroup per utterance, persistent over its levels,
//
//   forward   levels upwards; the owner lane of a node walks its in-arcs in the stored order, max then
//             sum, and carries the expected accuracy of the partial paths next to the log weight
//   backward  levels downwards over the out-arcs, likewise
//   arcs      arc_grad[a]: gamma(a) (mmi), gamma(a) (c(a) - c_avg) (smbr)
//   scatter   after a workgroup barrier: a lane owns a segment of the emission index (the emitting arcs
//             of one (frame, class) in ascending arc order), adds their arc_grad in fp64 in that order,
//             rounds once and stores the float.  No atomics anywhere on results: two runs, and any
//             workgroup size, give the same bits.
//
// Workgroup barriers only.  Every node, arc, level, graph, frame, class and segment index read from
// memory is range-checked before it is used: a violation raises the utterance's status word.  Every
// loop is bounded by the counts passed in.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

constexpr double DINF = __builtin_huge_val();

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// the batch, as csrc/lattice_dp.hip lays it out
struct Lat {
    int B;
    int64_t N, A, L, G, S;                  // nodes, arcs, levels of the batch; graph arcs and states
    const int64_t *node_off, *arc_off, *level_off;      // [B + 1]
    const int32_t *time, *state, *level;    // [N]; level: index into level_ptr
    const int32_t *src, *dst;               // [A] node indices of the utterance
    const int64_t *arc;                     // [A] arc index in the graph
    const int32_t *level_ptr, *level_node;  // [L + 1], [N]: the nodes of a level (batch indices)
    const int32_t *in_ptr, *in_arc;         // [N + 1], [A]: the in-arcs of a node (batch indices)
    const int32_t *out_ptr;                 // [N + 1]: the out-arcs of node v are [out_ptr[v], out_ptr[v + 1])
    const int32_t *frames, *reached;        // [B]
    const double *own_scale;                // [B] the scale of the search
    const float *w, *fin;                   // graph: [G], [S]
    const int32_t *il;                      // [G] input labels (class + 1; 0: epsilon)
    int start;
    int b_begin, b_count;
    int64_t n_begin, n_end;                 // node_off[b_begin], node_off[b_begin + b_count]: the workspace's nodes
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
    s.ok = t.n_begin <= s.n0 && s.n0 <= s.n1 && s.n1 <= t.n_end && s.n1 <= t.N && 0 <= s.a0 && s.a0 <= s.a1 &&
           s.a1 <= t.A && 0 <= s.l0 && s.l0 <= s.l1 && s.l1 <= t.L;
    return s;
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

struct TrainArgs {
    Lat t;
    double ac_scale, lm_scale, boost;       // ac_scale NaN: the utterance's own
    int criterion;                          // 0 mmi, 1 smbr
    const float *log_probs;                 // [T, B, C]
    const int32_t *ref;                     // [B, T] class per frame, -1 padding; null: no accuracies
    int T, C;
    int64_t E, NS;                          // emitting arcs and segments of the batch
    const int32_t *em_arc, *em_ptr;         // [E], [NS + 1]
    const int64_t *em_key, *em_off;         // [NS] offsets into occ, [B + 1] the segments of an utterance
    double *fwd, *bwd, *facc, *bacc;        // workspace [nodes of the launch]
    double *objective, *arc_grad;           // [B], [A]
    float *occ;                             // [T, B, C]
    int32_t *out_status;                    // [B]
};

__device__ __forceinline__ double lse_value(double m, double s) { return m == -DINF ? -DINF : m + log(s); }

// a - x for log weights: -inf as soon as the path weight is zero
__device__ __forceinline__ double log_times(double a, double x) { return (a == -DINF || x == DINF) ? -DINF : a - x; }

// The live cost of lattice arc with graph arc g into node d (a batch index inside the utterance) and its
// accuracy: x = fl(fl(fl(lm w) - fl(sc s)) + fl(boost acc)); this file is compiled with -ffp-contract=off.
// key: the arc's offset into occ, -1 for an epsilon arc.  False: a frame or class outside [T, B, C].
__device__ __forceinline__ bool live_cost(const TrainArgs &q, int b, int64_t g, int64_t d, double lm, double sc,
                                          double &x, double &acc, int64_t &key) {
    const Lat &t = q.t;
    const int32_t il = t.il[g];
    double s = 0.0;
    acc = 0.0;
    key = -1;
    if (il > 0) {
        const int32_t k = t.time[d];
        if (k < 1 || k > q.T || il > q.C) return false;
        key = ((int64_t)(k - 1) * t.B + b) * q.C + (il - 1);
        s = (double)q.log_probs[key];
        if (q.ref && q.ref[(int64_t)b * q.T + (k - 1)] == il - 1) acc = 1.0;
    }
    const double a = lm * (double)t.w[g];
    const double c = sc * s;
    const double e = q.boost * acc;
    x = (a - c) + e;
    return true;
}

template <int NT>
__global__ __launch_bounds__(NT) void lattice_seqtrain_kernel(const TrainArgs q) {
    const Lat &t = q.t;
    const int tid = threadIdx.x;
    const int b = t.b_begin + (int)blockIdx.x;
    __shared__ int64_t s_start;
    __shared__ unsigned long long s_emit, s_listed;
    if (tid == 0) s_start = INT64_MAX, s_emit = 0, s_listed = 0;
    __syncthreads();
    const bool smbr = q.criterion == 1;
    const double none = smbr ? 0.0 : -DINF;     // the objective of an utterance without a path
    const Span sp = span_of(t, b);
    bool fail = !sp.ok;
    if (!fail) fail = t.level_ptr[sp.l0] != sp.n0 || t.level_ptr[sp.l1] != sp.n1;
    int64_t g0 = 0, g1 = 0;                     // the utterance's segments
    if (!fail) {
        g0 = q.em_off[b], g1 = q.em_off[b + 1];
        fail = g0 < 0 || g0 > g1 || g1 > q.NS;
    }
    if (fail) {
        if (tid == 0) q.objective[b] = none, q.out_status[b] = 1;
        return;
    }
    double sc = q.ac_scale;
    if (sc != sc) sc = t.own_scale[b];
    const double lm = q.lm_scale;
    double *const fwd = q.fwd - t.n_begin, *const bwd = q.bwd - t.n_begin;
    double *const facc = q.facc - t.n_begin, *const bacc = q.bacc - t.n_begin;
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
                double m = is_start ? 0.0 : -DINF, s = 0.0, sa = 0.0;
                for (int pass = 0; pass < 2 && !bad; ++pass) {
                    if (pass == 1) {
                        if (m == -DINF) break;
                        s = is_start ? exp(0.0 - m) : 0.0;     // the empty path: accuracy 0
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
                        double x, acc;
                        int64_t key;
                        if (!live_cost(q, b, g, v, lm, sc, x, acc, key)) {
                            bad = true;
                            break;
                        }
                        const double term = log_times(fwd[u], x);
                        if (pass == 0) {
                            m = term > m ? term : m;
                        } else if (term != -DINF) {
                            const double p = exp(term - m);
                            s += p;
                            sa += p * (facc[u] + acc);
                        }
                    }
                }
                fwd[v] = lse_value(m, s);
                facc[v] = m == -DINF ? 0.0 : sa / s;    // sum of exp(term - fwd(v)) (facc(u) + acc)
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
                double m = stop, s = 0.0, sa = 0.0;
                for (int pass = 0; pass < 2 && !bad; ++pass) {
                    if (pass == 1) {
                        if (m == -DINF) break;
                        s = stop != -DINF ? exp(stop - m) : 0.0;       // stopping here: accuracy 0
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
                        double x, acc;
                        int64_t key;
                        if (!live_cost(q, b, g, d, lm, sc, x, acc, key)) {
                            bad = true;
                            break;
                        }
                        const double term = log_times(bwd[d], x);
                        if (pass == 0) {
                            m = term > m ? term : m;
                        } else if (term != -DINF) {
                            const double p = exp(term - m);
                            s += p;
                            sa += p * (bacc[d] + acc);
                        }
                    }
                }
                bwd[v] = lse_value(m, s);
                bacc[v] = m == -DINF ? 0.0 : sa / s;
            }
            dead = __syncthreads_or(bad) != 0;
            if (dead) break;
        }
    }
    const int64_t st = s_start;
    const bool have_start = !dead && st >= sp.n0 && st < sp.n1;
    const double z = have_start ? bwd[st] : -DINF;
    const double c_avg = (have_start && z != -DINF) ? bacc[st] : 0.0;
    // the arcs
    unsigned long long emitting = 0;
    for (int64_t a = sp.a0 + tid; a < sp.a1; a += NT) {
        double r = 0.0;
        if (!dead) {
            const int64_t u = sp.n0 + t.src[a], d = sp.n0 + t.dst[a], g = t.arc[a];
            double x, acc;
            int64_t key;
            if (u < sp.n0 || u >= sp.n1 || d < sp.n0 || d >= sp.n1 || g < 0 || g >= t.G) {
                bad = true;                     // an arc that no node's range covered
            } else if (!live_cost(q, b, g, d, lm, sc, x, acc, key)) {
                bad = true;
            } else {
                emitting += key >= 0 ? 1 : 0;
                if (z != -DINF) {
                    const double part = log_times(fwd[u], x);
                    if (part != -DINF && bwd[d] != -DINF) {
                        const double gamma = exp(part + bwd[d] - z);
                        r = smbr ? gamma * ((facc[u] + acc + bacc[d]) - c_avg) : gamma;
                    }
                }
            }
        }
        q.arc_grad[a] = r;
    }
    if (emitting) atomicAdd(&s_emit, emitting);
    dead = __syncthreads_or(bad) != 0 || dead;  // also makes arc_grad visible to every lane
    // the scatter: a lane per segment, its arcs in the stored (ascending) order
    if (!dead) {
        unsigned long long listed = 0;
        for (int64_t sg = g0 + tid; sg < g1; sg += NT) {
            const int64_t p0 = q.em_ptr[sg], p1 = q.em_ptr[sg + 1];
            const int64_t key = q.em_key[sg];
            if (p0 < 0 || p0 >= p1 || p1 > q.E || (sg > g0 && q.em_key[sg - 1] >= key)) {
                bad = true;                     // empty, out of range, or keys that do not ascend
                continue;
            }
            double sum = 0.0;
            int64_t prev = -1;
            for (int64_t p = p0; p < p1; ++p) {
                const int64_t a = q.em_arc[p];
                if (a < sp.a0 || a >= sp.a1 || a <= prev) {
                    bad = true;
                    break;
                }
                prev = a;
                const int64_t d = sp.n0 + t.dst[a], g = t.arc[a];       // both checked in the arc pass
                double x, acc;
                int64_t ka;
                if (!live_cost(q, b, g, d, lm, sc, x, acc, ka) || ka != key) {
                    bad = true;                 // not an emitting arc of this (frame, class)
                    break;
                }
                sum += q.arc_grad[a];
            }
            if (bad) continue;
            listed += (unsigned long long)(p1 - p0);
            q.occ[key] = (float)sum;            // key == ka: inside [T, B, C]
        }
        if (listed) atomicAdd(&s_listed, listed);
    }
    dead = __syncthreads_or(bad) != 0 || dead;
    if (!dead && s_emit != s_listed) dead = true;       // the index must list every emitting arc once
    if (tid == 0) {
        double obj = none;
        if (!dead && z != -DINF) obj = smbr ? c_avg : z;
        q.objective[b] = obj;
        q.out_status[b] = dead ? 1 : 0;
    }
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

bool threads_ok(int threads) { return threads == 0 || threads == 64 || threads == 128 || threads == 256; }

}  // namespace

extern "C" int asr_lattice_seqtrain_supported(int64_t N, int64_t A, int64_t L) { return sizes_ok(N, A, L) ? 1 : 0; }

extern "C" int64_t asr_lattice_seqtrain_workspace_bytes(int64_t num_nodes) {
    if (num_nodes < 0 || !sizes_ok(num_nodes, 0, 0)) return 0;
    return 4 * up16(num_nodes * 8) + 16;
}

extern "C" int asr_lattice_seqtrain_f64(
    int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, const int32_t *arc_ilabel,
    const float *log_probs, int T, int C, const int32_t *ref, int criterion, double boost, int64_t num_emitting,
    int64_t num_segments, const int32_t *em_arc, const int32_t *em_ptr, const int64_t *em_key,
    const int64_t *em_off, double *out_objective, double *out_arc_grad, float *out_occ, int32_t *out_status,
    void *workspace, int64_t workspace_bytes, void *stream) {
    (void)lat_lp;                               // the scores frozen at decode time are not read
    (void)arc_olabel;
    const int64_t S = num_states, G = num_graph_arcs, E = num_emitting, NS = num_segments;
    if (B < 0 || b_begin < 0 || b_count < 0 || (int64_t)b_begin + b_count > B) return ASR_EINVAL;
    if (N < 0 || A < 0 || L < 0 || S < 1 || G < 0 || start < 0 || start >= S) return ASR_EINVAL;
    if (T < 0 || C < 0 || (criterion != 0 && criterion != 1)) return ASR_EINVAL;
    if (!(boost >= 0.0) || boost == DINF || lm_scale != lm_scale) return ASR_EINVAL;
    if (E < 0 || E > A || NS < 0 || NS > E || !threads_ok(threads)) return ASR_EINVAL;
    if (!sizes_ok(N, A, L)) return ASR_EUNSUPPORTED;
    if (!offsets_ok(h_node_off, B, N) || !offsets_ok(h_arc_off, B, A) || !offsets_ok(h_level_off, B, L))
        return ASR_EINVAL;
    for (int b = 0; b < B; ++b) {               // a level holds a node; arcs need two nodes on two levels
        const int64_t n = h_node_off[b + 1] - h_node_off[b], l = h_level_off[b + 1] - h_level_off[b];
        if (l > n || (n > 0 && l < 1) || (h_arc_off[b + 1] > h_arc_off[b] && l < 2)) return ASR_EINVAL;
    }
    if (!node_off || !arc_off || !level_off || !level_ptr || !in_ptr || !out_ptr || !num_frames || !reached_final ||
        !own_scale || !final_cost || !em_ptr || !em_off)
        return ASR_EINVAL;
    if (N > 0 && (!node_time || !node_state || !node_level || !level_node)) return ASR_EINVAL;
    if (A > 0 && (!lat_src || !lat_dst || !lat_arc || !in_arc || !arc_weight || !arc_ilabel)) return ASR_EINVAL;
    if (E > 0 && (!em_arc || !em_key || !log_probs || !out_occ || T < 1 || C < 1 || B < 1)) return ASR_EINVAL;
    if (A > 0 && T > 0 && C > 0 && !log_probs) return ASR_EINVAL;
    if (!out_objective || !out_status || (A > 0 && !out_arc_grad)) return ASR_EINVAL;
    if (b_count == 0) return ASR_OK;
    const int64_t n = h_node_off[b_begin + b_count] - h_node_off[b_begin];
    const int64_t need = asr_lattice_seqtrain_workspace_bytes(n);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    TrainArgs q;
    q.t = Lat{B, N, A, L, G, S, node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst,
              lat_arc, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final, own_scale,
              arc_weight, final_cost, arc_ilabel, start, b_begin, b_count, h_node_off[b_begin],
              h_node_off[b_begin + b_count]};
    q.ac_scale = acoustic_scale;
    q.lm_scale = lm_scale;
    q.boost = boost;
    q.criterion = criterion;
    q.log_probs = log_probs;
    q.ref = ref;
    q.T = T, q.C = C;
    q.E = E, q.NS = NS;
    q.em_arc = em_arc, q.em_ptr = em_ptr, q.em_key = em_key, q.em_off = em_off;
    const int64_t stride = up16(n * 8);
    q.fwd = (double *)workspace;
    q.bwd = (double *)((uint8_t *)workspace + stride);
    q.facc = (double *)((uint8_t *)workspace + 2 * stride);
    q.bacc = (double *)((uint8_t *)workspace + 3 * stride);
    q.objective = out_objective;
    q.arc_grad = out_arc_grad;
    q.occ = out_occ;
    q.out_status = out_status;
    const dim3 grid((unsigned)b_count);
    switch (threads) {
    case 256: hipLaunchKernelGGL(lattice_seqtrain_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, q); break;
    case 128: hipLaunchKernelGGL(lattice_seqtrain_kernel<128>, grid, dim3(128), 0, (hipStream_t)stream, q); break;
    default: hipLaunchKernelGGL(lattice_seqtrain_kernel<64>, grid, dim3(64), 0, (hipStream_t)stream, q); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
