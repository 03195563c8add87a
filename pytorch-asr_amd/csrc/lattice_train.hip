// Sequence-discriminative training statistics over a batch of pruned lattices that stays on the device
// (include/asr_amd.h: asr_lattice_seqtrain_f64, asr_lattice_seqtrain_supported,
// asr_lattice_seqtrain_workspace_bytes): the denominator of lattice MMI and
// boosted MMI (log Z and the arc occupancies) and the sMBR objective (the expected frame accuracy and its
// derivative), with the arc scores read from the LIVE log_probs [T, B, C], and the occupancies delivered
// as the [T, B, C] tensor the encoder's backward takes.  LatticeBatch.seq_objective of
// att_speech/wfst_lattice.py is the numpy twin.
//
// The batch, its checked traversal and the host validation are csrc/lattice_batch.h's (nodes by (utterance,
// time, state), arcs by (utterance, source node, graph arc), the (time, epsilon rank) levels, the in-arcs of
// every node).  The kernel has the shape of csrc/lattice_dp.hip's lattice_posterior_kernel, one workgroup per
// utterance, persistent over its levels:
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
#include "lattice_batch.h"

namespace {

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
    bool fail = !sp.ok || !levels_cover(t, sp);
    int64_t g0 = 0, g1 = 0;                     // the utterance's segments
    if (!fail) {
        g0 = q.em_off[b], g1 = q.em_off[b + 1];
        fail = g0 < 0 || g0 > g1 || g1 > q.NS;
    }
    if (fail) {
        if (tid == 0) q.objective[b] = none, q.out_status[b] = 1;
        return;
    }
    const double sc = scale_of(t, b, q.ac_scale);
    const double lm = q.lm_scale;
    double *const fwd = q.fwd - t.n_begin, *const bwd = q.bwd - t.n_begin;
    double *const facc = q.facc - t.n_begin, *const bacc = q.bacc - t.n_begin;
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
                double m = is_start ? 0.0 : -DINF, s = 0.0, sa = 0.0;
                for (int pass = 0; pass < 2 && !bad; ++pass) {
                    if (pass == 1) {
                        if (m == -DINF) break;
                        s = is_start ? exp(0.0 - m) : 0.0;     // the empty path: accuracy 0
                    }
                    for (int64_t j = j0; j < j1; ++j) {
                        int64_t a, u, g;
                        if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
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
                int64_t j0, j1;
                const double en = end_cost(t, v, frames, reached, bad);
                const double stop = en < DINF ? 0.0 - lm * en : -DINF;
                if (!out_arcs_of(t, sp, v, j0, j1)) {
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
                        int64_t d, g;
                        if (!out_arc_at(t, sp, a, v, l, d, g)) {
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
            int64_t u, d, g, key;
            double x, acc;
            if (!arc_at(t, sp, a, u, d, g)) {
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
    const int64_t E = num_emitting, NS = num_segments;
    // ahead of fill_lat, whose ASR_EUNSUPPORTED for sizes must not hide these; its ASR_EINVAL for bad counts may
    // follow them, the code being the same.  lat_lp (the scores frozen at decode time) and arc_olabel are not read.
    if (T < 0 || C < 0 || (criterion != 0 && criterion != 1)) return ASR_EINVAL;
    if (!(boost >= 0.0) || boost == DINF || lm_scale != lm_scale) return ASR_EINVAL;
    if (E < 0 || E > A || NS < 0 || NS > E || !threads_ok(threads)) return ASR_EINVAL;
    TrainArgs q;
    const int rc = fill_lat(q.t, LAT_ILABEL, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off,
                            node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc,
                            lat_lp, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final,
                            own_scale, num_states, num_graph_arcs, arc_weight, arc_olabel, arc_ilabel, final_cost,
                            start);
    if (rc != ASR_OK) return rc;
    if (!em_ptr || !em_off) return ASR_EINVAL;
    if (E > 0 && (!em_arc || !em_key || !log_probs || !out_occ || T < 1 || C < 1 || B < 1)) return ASR_EINVAL;
    if (A > 0 && T > 0 && C > 0 && !log_probs) return ASR_EINVAL;
    if (!out_objective || !out_status || (A > 0 && !out_arc_grad)) return ASR_EINVAL;
    if (b_count == 0) return ASR_OK;
    const int64_t n = h_node_off[b_begin + b_count] - h_node_off[b_begin];
    const int64_t need = asr_lattice_seqtrain_workspace_bytes(n);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
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
    return launch_by_threads(threads, 64, b_count, stream, q, lattice_seqtrain_kernel<64>,
                             lattice_seqtrain_kernel<128>, lattice_seqtrain_kernel<256>);
}
