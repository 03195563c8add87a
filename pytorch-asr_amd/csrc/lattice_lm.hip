// Lattice o back-off n-gram LM on the device (include/asr_amd.h: asr_lattice_lmrescore_expand / _emit /
// _sweep and their _supported / _workspace_bytes; att_speech/lattice_lm.py states the
// semantics and holds the numpy twin that these kernels match bit for bit).
//
//   expand   one workgroup per utterance walks its (time, epsilon rank) levels upwards; a wave owns a node v
//            and pulls: for every in-arc and every LM state of the arc's source list it computes the LM step
//            (binary search in the LM's label-sorted CSR along the back-off chain) and collects the distinct
//            targets in LDS, then writes them sorted into v's list in the workspace (cap entries a node).
//            Sets only: no costs, no atomics on the lists, no dependence on the order of arrival.
//   emit     a thread per (lattice arc, LM state of its source): the step again, the position of the target in
//            the destination's sorted list, w' = fl32(fl64(w) + scale * c) by explicit round-to-nearest
//            intrinsics and a = -(fl32(acoustic scale) * lp).  The offsets are prefix sums made by the caller.
//   sweep    one workgroup per utterance over the expanded lattice: alpha upwards (in-arcs), the best end
//            node, beta downwards (out-arcs), the forward traceback by one lane, then the keep mask.  fp32,
//            one rounding per operation; minima only, so two runs give the same bits.
//
// All synchronise with workgroup barriers only.  Every index read from memory is range-checked before it is
// used; a violation raises the utterance's status word.  Every loop is bounded by the counts passed in.
#include "common.h"
#include "lattice_batch.h"                      // DINF, up16, sizes_ok; the argument structs here are this file's own

namespace {

constexpr float FINF = __builtin_huge_valf();
constexpr int MAX_STATES = ASR_LATTICE_LMRESCORE_MAX_STATES;
constexpr int NT = 256;
constexpr int NW = NT / ASR_WAVE;

struct Lm {
    int64_t Q, LA;                          // states, non-epsilon arcs
    const int32_t *ptr, *label, *dst;       // [Q + 1], [LA] sorted by (state, label), [LA]
    const double *weight;                   // [LA]
    const int32_t *bo_dst;                  // [Q]; -1: no back-off arc
    const double *bo_w;                     // [Q]
    int start;
    const int64_t *lmap;                    // [map_len] word of the graph -> label of the LM; <= 0: none
    int64_t map_len;
    double oov;
};

// The LM side of a lattice arc with output label o out of LM state q: false when the arc is dropped
// (out of vocabulary at an infinite oov cost); else qn is the LM state it leads to and c its LM cost.
__device__ __forceinline__ bool lm_next(const Lm &m, int q, int o, int &qn, double &c) {
    c = 0.0;
    qn = q;
    if (o == 0) return true;
    const int64_t l = (o > 0 && (int64_t)o < m.map_len) ? m.lmap[o] : -1;
    if (l > 0 && l < ((int64_t)1 << 31)) {
        const int want = (int)l;
        for (int64_t it = 0; it <= m.Q; ++it) {
            if (q < 0 || q >= m.Q) break;
            int64_t lo = m.ptr[q], hi = m.ptr[q + 1];
            if (lo < 0) lo = 0;
            if (hi > m.LA) hi = m.LA;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (m.label[mid] < want) lo = mid + 1;
                else hi = mid;
            }
            if (lo < m.LA && lo < m.ptr[q + 1] && m.label[lo] == want) {
                const int d = m.dst[lo];
                if (d < 0 || d >= m.Q) break;
                c = c + m.weight[lo];
                qn = d;
                return true;
            }
            const int bo = m.bo_dst[q];
            if (bo < 0 || bo >= m.Q) break;
            c = c + m.bo_w[q];
            q = bo;
            qn = q;
        }
    }
    c = m.oov;
    return m.oov < DINF;
}

struct ExpandArgs {
    Lm lm;
    int B, b_begin, b_count, cap;
    int64_t N, A, L, G, n_begin;
    const int64_t *node_off, *level_off;    // [B + 1]
    const int32_t *time, *state;            // [N]
    const int64_t *src, *arc;               // [A] batch node of the source; graph arc
    const int32_t *level_ptr, *level_node, *in_ptr, *in_arc;
    const int32_t *ol;                      // [G]
    int start;
    int32_t *cnt, *status, *list;           // [N], [B], workspace [nodes of the launch][cap]
};

__global__ __launch_bounds__(NT) void lmrescore_expand_kernel(const ExpandArgs q) {
    __shared__ int32_t s_list[NW][MAX_STATES];
    __shared__ int s_stop;
    const int tid = threadIdx.x, wave = tid / ASR_WAVE, lane = tid % ASR_WAVE;
    const int b = q.b_begin + (int)blockIdx.x;
    const int64_t n0 = q.node_off[b], n1 = q.node_off[b + 1], l0 = q.level_off[b], l1 = q.level_off[b + 1];
    if (tid == 0) s_stop = 0;
    __syncthreads();
    if (!(q.n_begin <= n0 && n0 <= n1 && n1 <= q.N && 0 <= l0 && l0 <= l1 && l1 <= q.L)) {
        if (tid == 0) atomicOr(&q.status[b], 2);
        return;
    }
    int32_t *mine = s_list[wave];
    const int cap = q.cap;
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t p0 = q.level_ptr[l], p1 = q.level_ptr[l + 1];
        if (p0 < 0 || p1 > q.N || p0 > p1) {
            if (tid == 0) s_stop = 2;
        } else {
            for (int64_t idx = p0 + wave; idx < p1; idx += NW) {
                const int64_t v = q.level_node[idx];
                int bad = 0;
                if (v < n0 || v >= n1) {
                    if (lane == 0) s_stop = 2;
                    continue;
                }
                int n = 0;
                if (q.time[v] == 0 && q.state[v] == q.start) {
                    if (lane == 0) mine[0] = q.lm.start;
                    n = 1;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                int64_t k0 = q.in_ptr[v], k1 = q.in_ptr[v + 1];
                if (k0 < 0 || k1 > q.A || k0 > k1) bad = 2, k1 = k0;
                for (int64_t k = k0; k < k1 && !bad; ++k) {
                    const int64_t j = q.in_arc[k];
                    if (j < 0 || j >= q.A) {
                        bad = 2;
                        break;
                    }
                    const int64_t u = q.src[j], a = q.arc[j];
                    if (u < n0 || u >= n1 || a < 0 || a >= q.G) {
                        bad = 2;
                        break;
                    }
                    const int o = q.ol[a];
                    int cu = q.cnt[u];
                    if (cu > cap) cu = cap;
                    const int32_t *lu = q.list + (u - q.n_begin) * cap;
                    for (int i0 = 0; i0 < cu && !bad; i0 += ASR_WAVE) {
                        const int i = i0 + lane;
                        bool ok = false;
                        int qn = 0;
                        double c;
                        if (i < cu) ok = lm_next(q.lm, lu[i], o, qn, c);
                        unsigned long long mask = __ballot(ok);
                        while (mask) {
                            const int lead = __ffsll((long long)mask) - 1;
                            mask &= mask - 1;
                            const int cand = __shfl(qn, lead, ASR_WAVE);
                            bool found = false;
                            for (int p = lane; p < n; p += ASR_WAVE) found |= mine[p] == cand;
                            if (__any(found)) continue;
                            if (n >= cap) {
                                bad = 1;
                                break;
                            }
                            if (lane == 0) mine[n] = cand;
                            ++n;
                            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                }
                if (bad) {
                    if (lane == 0) s_stop = bad;
                } else {
                    int32_t *lv = q.list + (v - q.n_begin) * cap;
                    for (int p = lane; p < n; p += ASR_WAVE) {
                        const int val = mine[p];
                        int r = 0;
                        for (int t = 0; t < n; ++t) r += mine[t] < val;
                        lv[r] = val;
                    }
                    if (lane == 0) q.cnt[v] = n;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        const int stop = s_stop;
        __syncthreads();
        if (stop) {
            if (tid == 0) atomicOr(&q.status[b], stop >= 2 ? 2 : 1);
            return;
        }
    }
}

struct EmitArgs {
    Lm lm;
    int cap;
    int64_t N, A, G, n0, n1, a0, a1, E, M;
    const int64_t *src, *dst, *arc_utt, *arc;       // [A]
    const float *lp;                                // [A]
    const double *own_scale;                        // [B]
    int B;
    const int32_t *ol;
    const float *w;
    double scale;
    const int32_t *cnt;                             // [N]
    const int64_t *e_off, *slot;                    // [n1 - n0 + 1], [a1 - a0 + 1]
    const int32_t *list;
    int32_t *n_q, *e_src, *e_dst, *e_q, *e_ok;
    double *e_c;
    float *e_w, *e_a;
};

// the last index i in [0, n] with off[i] <= t; off is ascending, off[0] = 0 and t < off[n]
__device__ __forceinline__ int64_t owner_of(const int64_t *off, int64_t n, int64_t t) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(NT) void lmrescore_emit_kernel(const EmitArgs q) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int cap = q.cap;
    if (t < q.E) {
        const int64_t vl = owner_of(q.e_off, q.n1 - q.n0, t);
        const int64_t i = t - q.e_off[vl];
        q.n_q[t] = (vl < q.n1 - q.n0 && i >= 0 && i < cap) ? q.list[vl * cap + i] : 0;
    }
    if (t >= q.M) return;
    const int64_t jl = owner_of(q.slot, q.a1 - q.a0, t);
    const int64_t i = t - q.slot[jl], j = q.a0 + jl;
    q.e_ok[t] = -1;
    if (jl >= q.a1 - q.a0 || i < 0 || i >= cap) return;
    const int64_t u = q.src[j], v = q.dst[j], a = q.arc[j], b = q.arc_utt[j];
    if (u < q.n0 || u >= q.n1 || v < q.n0 || v >= q.n1 || a < 0 || a >= q.G || b < 0 || b >= q.B) return;
    if (i >= q.cnt[u]) return;
    const int qq = q.list[(u - q.n0) * cap + i];
    int qn;
    double c;
    if (!lm_next(q.lm, qq, q.ol[a], qn, c)) {
        q.e_ok[t] = 0;
        return;
    }
    const int32_t *lv = q.list + (v - q.n0) * cap;
    int lo = 0, hi = q.cnt[v];
    if (hi > cap) hi = cap;
    const int n = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lv[mid] < qn) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= n || lv[lo] != qn) return;
    const int64_t es = q.e_off[u - q.n0] + i, ed = q.e_off[v - q.n0] + lo;
    q.e_src[t] = (int32_t)es;
    q.e_dst[t] = (int32_t)ed;
    q.e_q[t] = qq;
    q.e_c[t] = c;
    q.e_w[t] = __double2float_rn(__dadd_rn((double)q.w[a], __dmul_rn(q.scale, c)));
    q.e_a[t] = -__fmul_rn((float)q.own_scale[b], q.lp[j]);
    q.e_ok[t] = 1;
}

struct SweepArgs {
    int B;
    int64_t E, M, EL, N, S, Q;
    const int64_t *node_off, *arc_off, *level_off;  // [B + 1] of the expanded lattice
    const int32_t *level_ptr, *level_node, *in_ptr, *in_arc, *out_ptr;
    const int32_t *src, *dst;                       // [M] expanded nodes
    const float *w, *a;                             // [M]
    const int32_t *n_v, *n_q;                       // [E] lattice node (batch index), LM state
    const int32_t *time, *state;                    // [N]
    const int32_t *frames, *reached;                // [B]
    const float *fin;                               // [S]
    int start, lm_start;
    const double *final_star;                       // [Q]
    double scale;
    float beam;
    float *alpha, *beta;                            // [E]
    int32_t *keep;                                  // [M], zero on entry
    float *best;                                    // [B]
    int32_t *status;                                // [B]
};

template <int T>
__global__ __launch_bounds__(T) void lmrescore_sweep_kernel(const SweepArgs q) {
    __shared__ float s_best[T];
    __shared__ int64_t s_node[T];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int b = (int)blockIdx.x;
    const int64_t n0 = q.node_off[b], n1 = q.node_off[b + 1], a0 = q.arc_off[b], a1 = q.arc_off[b + 1];
    const int64_t l0 = q.level_off[b], l1 = q.level_off[b + 1];
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (!(0 <= n0 && n0 <= n1 && n1 <= q.E && 0 <= a0 && a0 <= a1 && a1 <= q.M && 0 <= l0 && l0 <= l1 && l1 <= q.EL)) {
        if (tid == 0) q.status[b] = 1;
        return;
    }
    const int frames = q.frames[b], reached = q.reached[b];
    // end costs into beta, seeds into alpha
    for (int64_t v = n0 + tid; v < n1; v += T) {
        const int64_t lv = q.n_v[v], lq = q.n_q[v];
        float end = FINF, al = FINF;
        if (lv < 0 || lv >= q.N || lq < 0 || lq >= q.Q) {
            s_bad = 1;
        } else {
            const int t = q.time[lv], s = q.state[lv];
            if (s < 0 || s >= q.S) {
                s_bad = 1;
            } else {
                if (t == frames) {
                    if (!reached) {
                        end = 0.f;
                    } else {
                        const double fg = (double)q.fin[s], fl = q.final_star[lq];
                        if (fg < DINF && fl < DINF) end = __double2float_rn(__dadd_rn(fg, __dmul_rn(q.scale, fl)));
                    }
                }
                if (t == 0 && s == q.start && lq == q.lm_start) al = 0.f;
            }
        }
        q.alpha[v] = al;
        q.beta[v] = end + 0.f;
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) q.status[b] = 1;
        return;
    }
    for (int64_t l = l0; l < l1; ++l) {
        int64_t p0 = q.level_ptr[l], p1 = q.level_ptr[l + 1];
        if (p0 < 0 || p1 > q.E || p0 > p1) p1 = p0, s_bad = 1;
        for (int64_t idx = p0 + tid; idx < p1; idx += T) {
            const int64_t v = q.level_node[idx];
            if (v < n0 || v >= n1) {
                s_bad = 1;
                continue;
            }
            float cur = q.alpha[v];
            int64_t k0 = q.in_ptr[v], k1 = q.in_ptr[v + 1];
            if (k0 < 0 || k1 > q.M || k0 > k1) k1 = k0, s_bad = 1;
            for (int64_t k = k0; k < k1; ++k) {
                const int64_t e = q.in_arc[k];
                if (e < a0 || e >= a1) {
                    s_bad = 1;
                    break;
                }
                const int64_t u = q.src[e];
                if (u < n0 || u >= n1) {
                    s_bad = 1;
                    break;
                }
                const float cand = ((q.alpha[u] + q.w[e]) + q.a[e]) + 0.f;
                if (cand < cur) cur = cand;
            }
            q.alpha[v] = cur;
        }
        __syncthreads();
    }
    if (s_bad) {
        if (tid == 0) q.status[b] = 1;
        return;
    }
    // the best end node: the smallest index among the minima of (alpha + end) + 0
    float bt = FINF;
    int64_t bv = -1;
    for (int64_t v = n0 + tid; v < n1; v += T) {
        const float tot = (q.alpha[v] + q.beta[v]) + 0.f;
        if (tot < bt) bt = tot, bv = v;         // ascending v: the first of equal totals stays
    }
    s_best[tid] = bt;
    s_node[tid] = bv;
    __syncthreads();
    for (int o = T / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const float x = s_best[tid + o];
            const int64_t xv = s_node[tid + o];
            if (xv >= 0 && (s_node[tid] < 0 || x < s_best[tid] || (x == s_best[tid] && xv < s_node[tid])))
                s_best[tid] = x, s_node[tid] = xv;
        }
        __syncthreads();
    }
    const float best = s_best[0];
    const int64_t end_node = s_node[0];
    __syncthreads();
    for (int64_t l = l1 - 1; l >= l0; --l) {
        const int64_t p0 = q.level_ptr[l], p1 = q.level_ptr[l + 1];
        for (int64_t idx = p0 + tid; idx < p1; idx += T) {
            const int64_t v = q.level_node[idx];
            float cur = q.beta[v];
            int64_t k0 = q.out_ptr[v], k1 = q.out_ptr[v + 1];
            if (k0 < a0 || k1 > a1 || k0 > k1) k1 = k0, s_bad = 1;
            for (int64_t e = k0; e < k1; ++e) {
                const int64_t d = q.dst[e];
                if (d < n0 || d >= n1) {
                    s_bad = 1;
                    break;
                }
                const float qv = ((q.w[e] + q.a[e]) + q.beta[d]) + 0.f;
                if (qv < cur) cur = qv;
            }
            q.beta[v] = cur;
        }
        __syncthreads();
    }
    if (s_bad) {
        if (tid == 0) q.status[b] = 1;
        return;
    }
    // the forward traceback: per node the first in-arc, in (source, graph arc) order, that attains alpha
    if (tid == 0 && end_node >= 0) {
        int64_t cur = end_node;
        for (int64_t step = l0; step <= l1; ++step) {
            const int64_t lv = q.n_v[cur];
            if (q.time[lv] == 0 && q.state[lv] == q.start && q.n_q[cur] == q.lm_start) break;
            const float want = q.alpha[cur];
            int64_t hit = -1;
            for (int64_t k = q.in_ptr[cur]; k < q.in_ptr[cur + 1]; ++k) {
                const int64_t e = q.in_arc[k];
                const float cand = ((q.alpha[q.src[e]] + q.w[e]) + q.a[e]) + 0.f;
                if (cand == want && cand < FINF) {
                    hit = e;
                    break;
                }
            }
            if (hit < 0) break;
            q.keep[hit] = 2;
            cur = q.src[hit];
        }
    }
    __syncthreads();
    const float limit = best + q.beam;
    for (int64_t e = a0 + tid; e < a1; e += T) {
        const float qv = ((q.w[e] + q.a[e]) + q.beta[q.dst[e]]) + 0.f;
        const float val = q.alpha[q.src[e]] + qv;
        q.keep[e] = ((val < FINF && val <= limit) || q.keep[e] == 2) ? 1 : 0;
    }
    if (tid == 0) q.best[b] = best;
}

int fill_lm(Lm &m, int64_t Q, int64_t LA, const int32_t *ptr, const int32_t *label, const int32_t *dst,
            const double *weight, const int32_t *bo_dst, const double *bo_w, int lm_start, const int64_t *lmap,
            int64_t map_len, double oov) {
    if (Q < 1 || LA < 0 || map_len < 0 || lm_start < 0 || lm_start >= Q || !sizes_ok(Q, LA, 0)) return ASR_EINVAL;
    if (!ptr || !bo_dst || !bo_w || (LA > 0 && (!label || !dst || !weight)) || (map_len > 0 && !lmap)) return ASR_EINVAL;
    if (oov != oov || oov == -DINF) return ASR_EINVAL;
    m.Q = Q, m.LA = LA, m.ptr = ptr, m.label = label, m.dst = dst, m.weight = weight, m.bo_dst = bo_dst, m.bo_w = bo_w;
    m.start = lm_start, m.lmap = lmap, m.map_len = map_len, m.oov = oov;
    return ASR_OK;
}

}  // namespace

extern "C" int asr_lattice_lmrescore_supported(int64_t N, int64_t A, int64_t L, int max_lm_states) {
    return sizes_ok(N, A, L) && max_lm_states >= 1 && max_lm_states <= MAX_STATES ? 1 : 0;
}

extern "C" int64_t asr_lattice_lmrescore_workspace_bytes(int64_t num_nodes, int max_lm_states) {
    if (num_nodes < 0 || max_lm_states < 1 || max_lm_states > MAX_STATES || !sizes_ok(num_nodes, 0, 0)) return 0;
    return up16(num_nodes * max_lm_states * 4) + 16;
}

extern "C" int asr_lattice_lmrescore_expand(
    int B, int b_begin, int b_count, int max_lm_states, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *node_off, const int64_t *level_off, const int32_t *node_time, const int32_t *node_state,
    const int64_t *src_global, const int64_t *lat_arc, const int32_t *level_ptr, const int32_t *level_node,
    const int32_t *in_ptr, const int32_t *in_arc, int64_t num_graph_arcs, const int32_t *arc_olabel, int start,
    int64_t lm_states, int64_t lm_arcs, const int32_t *lm_ptr, const int32_t *lm_label, const int32_t *lm_dst,
    const double *lm_weight, const int32_t *lm_bo_dst, const double *lm_bo_w, int lm_start, const int64_t *label_map,
    int64_t label_map_len, double oov_cost, int32_t *out_count, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream) {
    ExpandArgs q;
    if (B < 0 || b_begin < 0 || b_count < 0 || (int64_t)b_begin + b_count > B) return ASR_EINVAL;
    if (!sizes_ok(N, A, L)) return ASR_EUNSUPPORTED;
    if (max_lm_states < 1 || num_graph_arcs < 0 || start < 0) return ASR_EINVAL;
    if (max_lm_states > MAX_STATES) return ASR_EUNSUPPORTED;
    const int rc = fill_lm(q.lm, lm_states, lm_arcs, lm_ptr, lm_label, lm_dst, lm_weight, lm_bo_dst, lm_bo_w, lm_start,
                           label_map, label_map_len, oov_cost);
    if (rc != ASR_OK) return rc;
    if (b_count == 0) return ASR_OK;
    if (!h_node_off || !node_off || !level_off || !level_ptr || !in_ptr || !out_count || !out_status) return ASR_EINVAL;
    if (N > 0 && (!node_time || !node_state || !level_node)) return ASR_EINVAL;
    if (A > 0 && (!src_global || !lat_arc || !in_arc || !arc_olabel)) return ASR_EINVAL;
    const int64_t n_begin = h_node_off[b_begin], n = h_node_off[b_begin + b_count] - n_begin;
    if (n_begin < 0 || n < 0 || n_begin + n > N) return ASR_EINVAL;
    const int64_t need = asr_lattice_lmrescore_workspace_bytes(n, max_lm_states);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    q.B = B, q.b_begin = b_begin, q.b_count = b_count, q.cap = max_lm_states;
    q.N = N, q.A = A, q.L = L, q.G = num_graph_arcs, q.n_begin = n_begin;
    q.node_off = node_off, q.level_off = level_off, q.time = node_time, q.state = node_state;
    q.src = src_global, q.arc = lat_arc, q.level_ptr = level_ptr, q.level_node = level_node;
    q.in_ptr = in_ptr, q.in_arc = in_arc, q.ol = arc_olabel, q.start = start;
    q.cnt = out_count, q.status = out_status, q.list = (int32_t *)workspace;
    hipLaunchKernelGGL(lmrescore_expand_kernel, dim3((unsigned)b_count), dim3(NT), 0, (hipStream_t)stream, q);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

extern "C" int asr_lattice_lmrescore_emit(
    int B, int b_begin, int b_count, int max_lm_states, int64_t N, int64_t A, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *src_global, const int64_t *dst_global, const int64_t *arc_utt,
    const int64_t *lat_arc, const float *lat_lp, const double *own_scale, int64_t num_graph_arcs,
    const int32_t *arc_olabel, const float *arc_weight, int64_t lm_states, int64_t lm_arcs, const int32_t *lm_ptr,
    const int32_t *lm_label, const int32_t *lm_dst, const double *lm_weight, const int32_t *lm_bo_dst,
    const double *lm_bo_w, int lm_start, const int64_t *label_map, int64_t label_map_len, double oov_cost,
    double scale, const int32_t *count, const int64_t *node_slot, const int64_t *arc_slot, int64_t E, int64_t M,
    int32_t *out_lm_state, int32_t *out_src, int32_t *out_dst, int32_t *out_src_lm_state, double *out_lm_cost,
    float *out_weight, float *out_acoustic, int32_t *out_ok, const void *workspace, int64_t workspace_bytes,
    void *stream) {
    EmitArgs q;
    if (B < 0 || b_begin < 0 || b_count < 0 || (int64_t)b_begin + b_count > B) return ASR_EINVAL;
    if (!sizes_ok(N, A, 0) || !sizes_ok(E, M, 0)) return ASR_EUNSUPPORTED;
    if (max_lm_states < 1 || max_lm_states > MAX_STATES || num_graph_arcs < 0 || !(scale == scale)) return ASR_EINVAL;
    const int rc = fill_lm(q.lm, lm_states, lm_arcs, lm_ptr, lm_label, lm_dst, lm_weight, lm_bo_dst, lm_bo_w, lm_start,
                           label_map, label_map_len, oov_cost);
    if (rc != ASR_OK) return rc;
    if (b_count == 0 || (E == 0 && M == 0)) return ASR_OK;
    if (!h_node_off || !h_arc_off || !count || !node_slot || !arc_slot || !own_scale || !out_lm_state) return ASR_EINVAL;
    if (M > 0 && (!src_global || !dst_global || !arc_utt || !lat_arc || !lat_lp || !arc_olabel || !arc_weight ||
                  !out_src || !out_dst || !out_src_lm_state || !out_lm_cost || !out_weight || !out_acoustic || !out_ok))
        return ASR_EINVAL;
    q.n0 = h_node_off[b_begin], q.n1 = h_node_off[b_begin + b_count];
    q.a0 = h_arc_off[b_begin], q.a1 = h_arc_off[b_begin + b_count];
    if (q.n0 < 0 || q.n1 < q.n0 || q.n1 > N || q.a0 < 0 || q.a1 < q.a0 || q.a1 > A) return ASR_EINVAL;
    const int64_t need = asr_lattice_lmrescore_workspace_bytes(q.n1 - q.n0, max_lm_states);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    q.cap = max_lm_states, q.N = N, q.A = A, q.G = num_graph_arcs, q.E = E, q.M = M, q.B = B;
    q.src = src_global, q.dst = dst_global, q.arc_utt = arc_utt, q.arc = lat_arc, q.lp = lat_lp;
    q.own_scale = own_scale, q.ol = arc_olabel, q.w = arc_weight, q.scale = scale, q.cnt = count;
    q.e_off = node_slot, q.slot = arc_slot, q.list = (const int32_t *)workspace;
    q.n_q = out_lm_state, q.e_src = out_src, q.e_dst = out_dst, q.e_q = out_src_lm_state, q.e_ok = out_ok;
    q.e_c = out_lm_cost, q.e_w = out_weight, q.e_a = out_acoustic;
    const int64_t work = E > M ? E : M;
    hipLaunchKernelGGL(lmrescore_emit_kernel, dim3((unsigned)((work + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, q);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

extern "C" int asr_lattice_lmrescore_sweep(
    int B, int64_t E, int64_t M, int64_t EL, int64_t N, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr,
    const int32_t *in_arc, const int32_t *out_ptr, const int32_t *src, const int32_t *dst, const float *weight,
    const float *acoustic, const int32_t *lat_node, const int32_t *lm_state, const int32_t *node_time,
    const int32_t *node_state, const int32_t *num_frames, const int32_t *reached_final, int64_t num_states,
    const float *final_cost, int start, int64_t lm_states, const double *lm_final_star, int lm_start, double scale,
    double lattice_beam, int threads, float *out_alpha, float *out_beta, int32_t *out_keep, float *out_best,
    int32_t *out_status, void *stream) {
    if (B < 0 || E < 0 || M < 0 || EL < 0 || N < 0 || num_states < 1 || lm_states < 1) return ASR_EINVAL;
    if (!sizes_ok(E, M, EL) || !sizes_ok(N, 0, 0)) return ASR_EUNSUPPORTED;
    if (!(threads == 0 || threads == 64 || threads == 128 || threads == 256)) return ASR_EINVAL;
    if (!(scale == scale) || !(lattice_beam >= 0)) return ASR_EINVAL;
    if (B == 0) return ASR_OK;
    if (!node_off || !arc_off || !level_off || !level_ptr || !in_ptr || !out_ptr || !num_frames || !reached_final ||
        !final_cost || !lm_final_star || !out_best || !out_status)
        return ASR_EINVAL;
    if (E > 0 && (!level_node || !lat_node || !lm_state || !node_time || !node_state || !out_alpha || !out_beta))
        return ASR_EINVAL;
    if (M > 0 && (!in_arc || !src || !dst || !weight || !acoustic || !out_keep)) return ASR_EINVAL;
    SweepArgs q;
    q.B = B, q.E = E, q.M = M, q.EL = EL, q.N = N, q.S = num_states, q.Q = lm_states;
    q.node_off = node_off, q.arc_off = arc_off, q.level_off = level_off, q.level_ptr = level_ptr;
    q.level_node = level_node, q.in_ptr = in_ptr, q.in_arc = in_arc, q.out_ptr = out_ptr, q.src = src, q.dst = dst;
    q.w = weight, q.a = acoustic, q.n_v = lat_node, q.n_q = lm_state, q.time = node_time, q.state = node_state;
    q.frames = num_frames, q.reached = reached_final, q.fin = final_cost, q.start = start, q.lm_start = lm_start;
    q.final_star = lm_final_star, q.scale = scale, q.beam = (float)lattice_beam;
    q.alpha = out_alpha, q.beta = out_beta, q.keep = out_keep, q.best = out_best, q.status = out_status;
    const dim3 grid((unsigned)B);
    switch (threads) {
    case 64: hipLaunchKernelGGL(lmrescore_sweep_kernel<64>, grid, dim3(64), 0, (hipStream_t)stream, q); break;
    case 128: hipLaunchKernelGGL(lmrescore_sweep_kernel<128>, grid, dim3(128), 0, (hipStream_t)stream, q); break;
    default: hipLaunchKernelGGL(lmrescore_sweep_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, q); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
