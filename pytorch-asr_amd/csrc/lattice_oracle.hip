// The lattice oracle over a batch of pruned lattices that stays on the device (include/asr_amd.h:
// asr_lattice_oracle_i32, asr_lattice_oracle_supported, asr_lattice_oracle_workspace_bytes; DESIGN.md
// section 4.25): per utterance the complete path whose words are nearest to a reference in word edit
// distance, with the split into substitutions, insertions and deletions, the path's words and cost and the
// frame every reference word was aligned to.  LatticeBatch.oracle of att_speech/wfst_lattice.py is the numpy
// twin; the distances are int32, so both agree with ==.
//
// The batch, its checked traversal and the host validation are csrc/lattice_batch.h's (nodes by (utterance, time,
// state), arcs by (utterance, source node, graph arc), the (time, epsilon rank) levels, the in-arcs of every
// node); the shape of the kernel is that of csrc/lattice_dp.hip's: one workgroup per utterance, persistent over
// its levels; a wave owns a node of a level and takes its in-arcs in turn; its lanes run over the reference
// positions q = 0 .. R in rounds of 64.  The deletion chain D(v, q) = min(D0(v, q), D(v, q - 1) + 1) is q + the
// running minimum of D0(v, i) - i: a wave-level prefix minimum with a carry between the rounds.  The rows D(v, .)
// stay in the workspace; one wave walks them back from the end node, a lane per in-arc, the first arc that
// attains D(v, q) found by ballot.
//
// Workgroup barriers only.  Every node, arc, level and graph index read from memory is range-checked before
// it is used: a violation raises the utterance's status word.  Every loop is bounded by the counts passed in.
#include "common.h"
#include "lattice_batch.h"

namespace {

constexpr int ORACLE_MAX_WORDS = ASR_LATTICE_ORACLE_MAX_WORDS;
constexpr int32_t UNREACHABLE = 1 << 30;        // U: no path; every sum is clamped to it

struct OracleArgs {
    Lat t;
    double ac_scale, lm_scale;              // ac_scale NaN: the utterance's own
    const int32_t *ref_words, *ref_nwords;  // [B][W], [B]
    int W, C;                               // C = W + 1 columns a node
    int32_t *D;                             // workspace [nodes of the launch][C]
    int32_t *out_errors, *out_counts;       // [B], [B][4]: sub, ins, del, cor
    int32_t *out_nwords, *out_words;        // [B], [L]
    int32_t *out_frames;                    // [B][W]
    double *out_cost;                       // [B]
    int32_t *out_status;                    // [B]
};

__device__ __forceinline__ int32_t clamp_u(int32_t v) { return v < UNREACHABLE ? v : UNREACHABLE; }

// c_j(q) of an in-arc with word w from the row of its source; rq = r_q (q >= 1)
__device__ __forceinline__ int32_t arc_value(const int32_t *du, int32_t w, int q, int32_t rq) {
    const int32_t stay = du[q];
    if (w == 0) return stay;
    int32_t c = clamp_u(stay + 1);
    if (q >= 1) {
        const int32_t diag = clamp_u(du[q - 1] + (w != rq ? 1 : 0));
        c = diag < c ? diag : c;
    }
    return c;
}

template <int NT>
__global__ __launch_bounds__(NT) void lattice_oracle_kernel(const OracleArgs q) {
    const Lat &t = q.t;
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = t.b_begin + (int)blockIdx.x;
    const int W = q.W, C = q.C;
    __shared__ unsigned long long s_start, s_best;
    if (tid == 0) s_start = ~0ull, s_best = ~0ull;
    __syncthreads();
    const Span sp = span_of(t, b);
    const int R = q.ref_nwords[b];
    if (!sp.ok || R < 0 || R > W || !levels_cover(t, sp)) {     // uniform: every lane read the same words
        if (tid == 0) {
            q.out_errors[b] = -1, q.out_nwords[b] = 0, q.out_cost[b] = DINF, q.out_status[b] = 1;
            for (int k = 0; k < 4; ++k) q.out_counts[4 * (int64_t)b + k] = 0;
        }
        return;
    }
    const double sc = scale_of(t, b, q.ac_scale);
    const double lm = q.lm_scale;
    const int frames = t.frames[b], reached = t.reached[b];
    const int64_t nlev = sp.l1 - sp.l0;
    int32_t *const D = q.D - t.n_begin * C;     // indexed by batch node * C + position
    const int32_t *const ref = q.ref_words + (int64_t)b * W;
    bool bad = false, dead = false;

    for (int64_t v = sp.n0 + tid; v < sp.n1; v += NT)
        if (t.time[v] == 0 && t.state[v] == t.start) atomicMin(&s_start, (unsigned long long)v);
    __syncthreads();
    const int64_t st = s_start == ~0ull ? -1 : (int64_t)s_start;
    const int rounds = (R + 1 + 63) >> 6;

    // forward, levels upwards: a wave owns a node and takes its in-arcs in turn
    for (int64_t l = sp.l0; l < sp.l1 && st >= 0; ++l) {
        const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
        if (!level_range(e0, e1, sp.n0, sp.n1)) {
            bad = true;
        } else {
            for (int64_t e = e0 + wave; e < e1; e += NW) {      // everything but the position is uniform in the wave
                int64_t v, j0, j1;
                if (!node_at(t, sp, e, l, v) || !in_arcs_of(t, sp, v, j0, j1)) {
                    bad = true;
                    continue;
                }
                int32_t *const dv = D + v * C;
                if (v == st) {                  // the start row; arcs into the start node are ignored
                    for (int k = lane; k <= R; k += 64) dv[k] = k;
                    continue;
                }
                int32_t carry = INT32_MAX;      // min over the rounds below of D0(v, i) - i
                for (int r = 0; r < rounds && !bad; ++r) {
                    const int qq = lane + 64 * r;
                    const bool act = qq <= R;
                    const int32_t rq = (act && qq >= 1) ? ref[qq - 1] : 0;
                    int32_t m = UNREACHABLE;
                    for (int64_t j = j0; j < j1; ++j) {
                        int64_t a, u, g;
                        if (!in_arc_at(t, sp, j, v, l, a, u, g)) {
                            bad = true;
                            break;
                        }
                        if (act) {
                            const int32_t c = arc_value(D + u * C, t.ol[g], qq, rq);
                            m = c < m ? c : m;
                        }
                    }
                    int32_t x = act ? m - qq : INT32_MAX;
                    for (int d = 1; d < 64; d <<= 1) {          // prefix minimum over the lanes
                        const int32_t o = __shfl_up(x, d);
                        if (lane >= d && o < x) x = o;
                    }
                    if (carry < x) x = carry;
                    carry = __shfl(x, 63);
                    if (act) dv[qq] = clamp_u(x + qq);
                }
            }
        }
        dead = __syncthreads_or(bad) != 0;      // also makes the level's rows visible to every wave
        if (dead) break;
    }

    // the end node: the least D(v, R), the smallest node among the minima
    if (!dead && st >= 0) {
        for (int64_t v = sp.n0 + tid; v < sp.n1; v += NT) {
            if (!(end_cost(t, v, frames, reached, bad) < DINF)) continue;
            const int32_t d = D[v * C + R];
            if (d >= 0 && d < UNREACHABLE)
                atomicMin(&s_best, ((unsigned long long)(uint32_t)d << 32) | (unsigned long long)(v - sp.n0));
        }
    }
    dead = __syncthreads_or(bad) != 0 || dead;
    const unsigned long long best = s_best;
    const bool have = !dead && st >= 0 && best != ~0ull;
    int32_t errors = -1, n_sub = 0, n_ins = 0, n_del = 0, n_cor = 0, nw = 0;
    double cost = DINF;

    // the traceback by one wave: a lane per in-arc, the first hit in the stored order by ballot
    if (wave == 0 && have) {
        const int64_t vstar = sp.n0 + (int64_t)(best & 0xFFFFFFFFull);
        errors = (int32_t)(best >> 32);
        int32_t *const slots = q.out_words + sp.l0;     // the path's arcs from the back, then its words from the front
        int32_t *const fr = q.out_frames + (int64_t)b * W;
        int64_t v = vstar, k = 0;
        int qq = R;
        bool done = false;
        for (int64_t step = 0; step <= nlev + R && !bad; ++step) {      // every step lowers the level or q
            if (v == st) {
                done = true;
                break;
            }
            const int64_t lv = t.level[v];
            int64_t j0, j1;
            if (lv < sp.l0 || lv >= sp.l1 || !in_arcs_of(t, sp, v, j0, j1)) {
                bad = true;
                break;
            }
            const int32_t target = D[v * C + qq];
            const int32_t rq = qq >= 1 ? ref[qq - 1] : 0;
            int32_t al = -1, ul = -1, w = 0;
            for (int64_t jb = j0; jb < j1 && al < 0; jb += 64) {
                const int64_t j = jb + lane;
                int32_t my_a = -1, my_u = -1, my_w = 0;
                bool hit = false, wrong = false;
                if (j < j1) {
                    int64_t a, u, g;
                    if (!in_arc_at(t, sp, j, v, lv, a, u, g)) {
                        wrong = true;
                    } else {
                        my_a = (int32_t)(a - sp.a0), my_u = (int32_t)(u - sp.n0), my_w = t.ol[g];
                        hit = arc_value(D + u * C, my_w, qq, rq) == target;
                    }
                }
                if (__ballot(wrong) != 0ull) {
                    bad = true;
                    break;
                }
                const unsigned long long mask = __ballot(hit);
                if (mask != 0ull) {
                    const int first = __ffsll((long long)mask) - 1;
                    al = __shfl(my_a, first), ul = __shfl(my_u, first), w = __shfl(my_w, first);
                }
            }
            if (bad) break;
            if (al < 0) {                       // no in-arc attains D(v, q): r_q is deleted
                if (qq < 1) {
                    bad = true;
                    break;
                }
                if (lane == 0) fr[qq - 1] = -1;
                ++n_del, --qq;
                continue;
            }
            const int64_t u = sp.n0 + ul;
            if (k >= nlev) {                    // a path has at most one arc per level
                bad = true;
                break;
            }
            if (lane == 0) slots[nlev - 1 - k] = al;
            ++k;
            if (w != 0 && qq >= 1 && clamp_u(D[u * C + qq - 1] + (w != rq ? 1 : 0)) == target) {
                if (w == rq)
                    ++n_cor;
                else
                    ++n_sub;
                if (lane == 0) fr[qq - 1] = t.time[v];
                --qq;
            } else if (w != 0) {
                ++n_ins;
            }
            v = u;
        }
        if (!done) bad = true;
        if (!bad) {
            for (int i = lane; i < qq; i += 64) fr[i] = -1;     // at the start node the rest is deleted
            n_del += qq;
            if (lane == 0) {                    // forwards: the cost as the n-best read-out sums it, and the words
                double g = 0.0;
                for (int64_t i = 0; i < k; ++i) {
                    const int64_t a = sp.a0 + slots[nlev - k + i];      // checked when it was written
                    const int64_t ga = t.arc[a];
                    g = g + arc_cost(lm, sc, t.w[ga], t.lp[a]);
                    const int32_t word = t.ol[ga];
                    if (word != 0) slots[nw++] = word;          // nw <= i: never over an arc still to be read
                }
                cost = g + scaled_end(t, vstar, frames, reached, lm, bad);
            }
        }
    }
    dead = __syncthreads_or(bad) != 0 || dead;
    if (tid == 0) {
        const bool ok = have && !dead;
        q.out_errors[b] = ok ? errors : -1;
        q.out_counts[4 * (int64_t)b] = ok ? n_sub : 0;
        q.out_counts[4 * (int64_t)b + 1] = ok ? n_ins : 0;
        q.out_counts[4 * (int64_t)b + 2] = ok ? n_del : 0;
        q.out_counts[4 * (int64_t)b + 3] = ok ? n_cor : 0;
        q.out_nwords[b] = ok ? nw : 0;
        q.out_cost[b] = ok ? cost : DINF;
        q.out_status[b] = dead ? 1 : 0;
    }
}

}  // namespace

extern "C" int asr_lattice_oracle_supported(int64_t N, int64_t A, int64_t L, int max_words) {
    return sizes_ok(N, A, L) && max_words >= 1 && max_words <= ORACLE_MAX_WORDS && L + max_words < UNREACHABLE ? 1 : 0;
}

extern "C" int64_t asr_lattice_oracle_workspace_bytes(int64_t num_nodes, int max_words) {
    if (num_nodes < 0 || max_words < 1 || max_words > ORACLE_MAX_WORDS || !sizes_ok(num_nodes, 0, 0)) return 0;
    return up16(num_nodes * ((int64_t)max_words + 1) * 4) + 16;
}

extern "C" int asr_lattice_oracle_i32(
    int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, const int32_t *ref_words,
    const int32_t *ref_num_words, int max_words, int32_t *out_errors, int32_t *out_counts, int32_t *out_num_words,
    int32_t *out_words, int32_t *out_ref_frames, double *out_cost, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream) {
    OracleArgs q;
    const int rc = fill_lat(q.t, LAT_LP | LAT_OLABEL, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off,
                            node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc,
                            lat_lp, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final,
                            own_scale, num_states, num_graph_arcs, arc_weight, arc_olabel, nullptr, final_cost, start);
    if (rc != ASR_OK) return rc;
    if (max_words < 1 || !threads_ok(threads)) return ASR_EINVAL;
    if (max_words > ORACLE_MAX_WORDS || L + max_words >= UNREACHABLE) return ASR_EUNSUPPORTED;
    if (b_count == 0) return ASR_OK;
    if (!ref_words || !ref_num_words || !out_errors || !out_counts || !out_num_words || !out_ref_frames || !out_cost ||
        !out_status || (L > 0 && !out_words))
        return ASR_EINVAL;
    const int64_t n = h_node_off[b_begin + b_count] - h_node_off[b_begin];
    const int64_t need = asr_lattice_oracle_workspace_bytes(n, max_words);
    if (need <= 0 || !workspace || workspace_bytes < need) return ASR_EINVAL;
    q.ac_scale = acoustic_scale;
    q.lm_scale = lm_scale;
    q.ref_words = ref_words;
    q.ref_nwords = ref_num_words;
    q.W = max_words;
    q.C = max_words + 1;
    q.D = (int32_t *)workspace;
    q.out_errors = out_errors;
    q.out_counts = out_counts;
    q.out_nwords = out_num_words;
    q.out_words = out_words;
    q.out_frames = out_ref_frames;
    q.out_cost = out_cost;
    q.out_status = out_status;
    // threads 0: four waves, four nodes of a level at a time
    return launch_by_threads(threads, 256, b_count, stream, q, lattice_oracle_kernel<64>, lattice_oracle_kernel<128>,
                             lattice_oracle_kernel<256>);
}
