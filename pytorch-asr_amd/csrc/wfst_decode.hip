// Beam-pruned Viterbi search over one shared decoding graph (include/asr_amd.h: asr_wfst_decode_f32,
// asr_wfst_decode_supported, asr_wfst_decode_workspace_bytes).
//
// The reference scores its systems by dumping log-probs and running Kaldi's decode-faster over a
// tropical decoding graph with a beam (egs/wsj/ctc_kaldi_decode.sh:141-147).  This is that search
// as frame-synchronous token passing with the order-independent semantics of DESIGN.md section 4.19:
// every arithmetic step is one fp32 operation without contraction, a state's cost is the minimum of
// its proposals, and of equal proposals the smallest arc index wins.  Both fall out of ONE 64-bit
// unsigned atomic minimum over (order-preserving bits of the cost) << 32 | arc index.
//
// One workgroup owns one utterance for all of its frames and synchronises with workgroup barriers
// only.  Per utterance the workspace holds a table of one such 64-bit word per graph state (all ones
// = no token), a table of record indices per state, three token lists and the back-pointer log.  A
// frame:
//   stage    the frame's C scaled scores -(acoustic_scale * lp) go to LDS from registers that were
//            loaded one frame earlier;
//   expand   NT tokens at a time (NT = the workgroup's threads, pick_threads in wfst_search.h): a block-wide
//            prefix sum of their out-degrees, then every lane takes arcs j, j + NT, ... of the
//            chunk and finds its token by binary search over the prefix
//            sums, so a state with thousands of arcs is spread over the whole workgroup;
//   propose  a plain read of the destination's word skips proposals that cannot win (the word only
//            falls during a phase), the others go through the atomic; the lane that finds the word
//            empty appends the state to the new list;
//   prune    against the best emitting cost + beam while compacting the list; pruned words are emptied;
//   closure  the epsilon levels in rank order, over the states of the list whose rank is the level's
//            (a state's cost is final before its level), through a CSR of the epsilon arcs alone;
//   log      every token that exists after the closure gets a record (arc, record of the source's
//            token): the source of an epsilon arc may be pruned below while its target survives;
//   prune    against the best cost + beam into the next frame's list (state, cost); every word that
//            was touched is emptied, so the table is clean for the next frame.
// Every loop is bounded by the frame count, the number of epsilon ranks, the list lengths and the
// arc counts of the listed states; an utterance that outgrows a list or the log raises its flag and
// ends (the caller redoes it on the host).  One lane walks the records back at the end.
#include "wfst_search.h"
#include "../../include/asr_amd.h"

namespace {

struct Params {
    Graph g;
    const float *lp;            // lp[t * frame_stride + b * C + c]
    int64_t frame_stride;
    const int32_t *lens;
    int T, B, C;
    float beam, scale;
    int allow_partial;
    uint32_t list_cap, log_cap;
    int word_cap;
    float *out_cost;
    int32_t *out_final, *out_align, *out_nact, *out_words, *out_nwords, *out_overflow;
    unsigned long long *tab;    // [B][N]
    uint32_t *slot;             // [B][N]
    uint32_t *lists;            // [B][5][list_cap]
    uint32_t *rec;              // [B][2][log_cap]
};

template <int NT>
__global__ __launch_bounds__(NT) void wfst_decode_kernel(const Params p) {
    constexpr int PRE = MAX_C / NT;                 // score registers per lane
    extern __shared__ __align__(16) float sc[];     // [C] scaled scores of the frame
    __shared__ Shared<NT> sh;
    const Graph &g = p.g;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = p.T, C = p.C;
    int32_t *const align = p.out_align + (int64_t)b * T;
    int32_t *const nact = p.out_nact + (int64_t)b * T;
    for (int t = tid; t < T; t += NT) {
        align[t] = -1;
        nact[t] = 0;
    }
    if (tid == 0) {
        p.out_cost[b] = INFINITY;
        p.out_final[b] = 0;
        p.out_nwords[b] = 0;
        p.out_overflow[b] = 0;
    }
    const int n = p.lens[b];
    if (n < 1 || n > T) return;

    unsigned long long *const tab = p.tab + (int64_t)b * g.N;
    uint32_t *const slot = p.slot + (int64_t)b * g.N;
    const uint32_t cap = p.list_cap;
    uint32_t *const cur_s = p.lists + (int64_t)b * 5 * cap;
    float *const cur_c = (float *)(cur_s + cap);
    uint32_t *const raw_s = cur_s + 2 * (int64_t)cap;
    uint32_t *const new_s = cur_s + 3 * (int64_t)cap;
    uint32_t *const new_p = cur_s + 4 * (int64_t)cap;
    uint32_t *const rec_a = p.rec + (int64_t)b * 2 * p.log_cap;
    uint32_t *const rec_p = rec_a + p.log_cap;
    const float *const col = p.lp + (int64_t)b * C;

    float pre[PRE];
    auto load_row = [&](int t) {
        const float *const row = col + p.frame_stride * t;
#pragma unroll
        for (int k = 0; k < PRE; ++k) {
            const int c = tid + k * NT;
            pre[k] = c < C ? row[c] : 0.f;
        }
    };
    load_row(0);
    if (tid == 0) {
        sh.ovf = 0;
        sh.rec_used = 0;
        sh.cnt_a = 0;
        sh.cnt_b = 1;
        sh.min_key = NONE;
        new_s[0] = g.start;
        new_p[0] = NONE;
        tab[g.start] = ((unsigned long long)fkey(0.f) << 32) | NONE;
    }
    __syncthreads();
    uint32_t ncur = 0;

    for (int t = -1; t < n; ++t) {
        if (t >= 0) {
#pragma unroll
            for (int k = 0; k < PRE; ++k) {
                const int c = tid + k * NT;
                if (c < C) sc[c] = -__fmul_rn(p.scale, pre[k]);
            }
            if (t + 1 < n) load_row(t + 1);
            __syncthreads();                        // scores staged; cnt_a == 0, cnt_b == 0, min_key == NONE
            expand<NT, false>(g, sh, sc, C, cur_s, cur_c, ncur, 0, tab, raw_s, nullptr, &sh.cnt_a, cap);
            __syncthreads();
            if (sh.ovf) break;
            const uint32_t nraw = sh.cnt_a;
            uint32_t m = NONE;
            for (uint32_t i = tid; i < nraw; i += NT) m = min(m, (uint32_t)(tab[raw_s[i]] >> 32));
            m = wave_min_u32(m);
            if ((tid & 63) == 0 && m != NONE) atomicMin(&sh.min_key, m);
            __syncthreads();
            const float thr = __fadd_rn(keyf(sh.min_key), p.beam);
            for (uint32_t i = tid; i < nraw; i += NT) {
                const uint32_t s = raw_s[i];
                const unsigned long long k = tab[s];
                if (keyf((uint32_t)(k >> 32)) <= thr) {
                    const uint32_t pos = atomicAdd(&sh.cnt_b, 1u);      // <= nraw <= cap
                    new_s[pos] = s;
                    new_p[pos] = slot[g.src[(uint32_t)k]];              // the source survived the previous frame
                } else {
                    tab[s] = EMPTY;
                }
            }
        }
        for (int level = 0; level < g.num_ranks; ++level) {
            __syncthreads();
            // a level that outgrew the list has counted past its end: the entries beyond cap were never
            // written, so the closure stops here (uniform) and the count is never taken above cap
            const bool full = sh.ovf != 0;
            const uint32_t cnt = min(sh.cnt_b, cap);
            __syncthreads();
            if (full) break;
            expand<NT, true>(g, sh, sc, C, new_s, nullptr, cnt, level, tab, new_s, new_p, &sh.cnt_b, cap);
        }
        __syncthreads();
        if (sh.ovf) break;
        const uint32_t n2 = sh.cnt_b, rec_base = sh.rec_used;
        if (n2 > p.log_cap - rec_base) {            // uniform
            if (tid == 0) sh.ovf = 1;
            __syncthreads();
            break;
        }
        if (tid == 0) {
            sh.min_key = NONE;
            sh.cnt_a = 0;
        }
        __syncthreads();
        {
            uint32_t m = NONE;
            for (uint32_t i = tid; i < n2; i += NT) {
                const uint32_t s = new_s[i];
                slot[s] = rec_base + i;
                m = min(m, (uint32_t)(tab[s] >> 32));
            }
            m = wave_min_u32(m);
            if ((tid & 63) == 0 && m != NONE) atomicMin(&sh.min_key, m);
        }
        __syncthreads();
        const bool last = t == n - 1;
        const float thr = __fadd_rn(keyf(sh.min_key), p.beam);
        for (uint32_t i = tid; i < n2; i += NT) {
            const uint32_t s = new_s[i];
            const unsigned long long k = tab[s];
            const uint32_t a = (uint32_t)k;
            uint32_t prev = NONE;
            if (a != NONE) prev = g.il[a] == 0 ? slot[g.src[a]] : new_p[i];
            rec_a[rec_base + i] = a;
            rec_p[rec_base + i] = prev;
            const float c = keyf((uint32_t)(k >> 32));
            if (last || c <= thr) {
                const uint32_t pos = atomicAdd(&sh.cnt_a, 1u);          // <= n2 <= cap
                cur_s[pos] = s;
                cur_c[pos] = c;
            }
            tab[s] = EMPTY;
        }
        __syncthreads();
        ncur = sh.cnt_a;
        __syncthreads();
        if (tid == 0) {
            sh.rec_used = rec_base + n2;
            sh.cnt_a = 0;
            sh.cnt_b = 0;
            sh.min_key = NONE;
            if (t >= 0) nact[t] = (int32_t)ncur;
        }
    }
    if (sh.ovf) {       // uniform: every way to the flag passes a barrier
        if (tid == 0) p.out_overflow[b] = 1;
        return;
    }

    // the best final state, or the best state: ties to the smallest state id
    if (tid == 0) sh.best_final = sh.best_any = EMPTY;
    __syncthreads();
    for (uint32_t i = tid; i < ncur; i += NT) {
        const uint32_t s = cur_s[i];
        const float c = cur_c[i], f = g.fin[s];
        atomicMin(&sh.best_any, ((unsigned long long)fkey(c) << 32) | s);
        if (f < INFINITY) {
            const float tot = __fadd_rn(__fadd_rn(c, f), 0.f);
            if (tot < INFINITY) atomicMin(&sh.best_final, ((unsigned long long)fkey(tot) << 32) | s);
        }
    }
    __syncthreads();
    if (tid != 0) return;
    const bool reached = sh.best_final != EMPTY;
    const unsigned long long best = reached ? sh.best_final : sh.best_any;
    if (best == EMPTY || (!reached && !p.allow_partial)) return;
    int32_t *const words = p.out_words + (int64_t)b * p.word_cap;
    const uint32_t total = sh.rec_used;
    uint32_t r = slot[(uint32_t)best];
    int t = n - 1, nw = 0;
    for (uint32_t step = 0; step < total && r < total; ++step) {
        const uint32_t a = rec_a[r];
        if (a == NONE) break;                       // the start token
        const int il = g.il[a], ol = g.ol[a];
        if (il > 0) {
            if (t >= 0) align[t] = il;
            --t;
        }
        if (ol != 0) {
            if (nw < p.word_cap) words[nw] = ol;    // last word first
            ++nw;
        }
        r = rec_p[r];
    }
    if (nw > p.word_cap) {
        p.out_overflow[b] = 1;
        return;
    }
    p.out_nwords[b] = nw;
    p.out_cost[b] = keyf((uint32_t)(best >> 32));
    p.out_final[b] = reached ? 1 : 0;
}

struct Layout {
    int64_t tab, slot, lists, rec, total;
};

Layout layout(int64_t N, int64_t B, int64_t list_cap, int64_t log_cap) {
    Layout l;
    l.tab = 0;
    l.slot = up16(B * N * 8);
    l.lists = l.slot + up16(B * N * 4);
    l.rec = l.lists + up16(B * 5 * list_cap * 4);
    l.total = l.rec + up16(B * 2 * log_cap * 4);
    return l;
}

bool caps_ok(int64_t list_cap, int64_t log_cap) {
    return list_cap >= 1 && list_cap < ((int64_t)1 << 31) && log_cap >= 1 && log_cap < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int asr_wfst_decode_supported(int64_t N, int64_t A, int C, int T) { return shapes_ok(N, A, C, T) ? 1 : 0; }

extern "C" int64_t asr_wfst_decode_workspace_bytes(int64_t N, int B, int64_t list_cap, int64_t log_cap) {
    if (N < 1 || B < 1 || !caps_ok(list_cap, log_cap)) return 0;
    return layout(N, B, list_cap, log_cap).total;
}

extern "C" int asr_wfst_decode_f32(const float *lp, int64_t frame_stride, const int32_t *lens, int T, int B, int C,
                                   int64_t N, int64_t A, const uint32_t *arc_ptr, const int32_t *arc_src,
                                   const int32_t *arc_dst, const int32_t *arc_ilabel, const int32_t *arc_olabel,
                                   const float *arc_weight, const float *final_cost, const uint32_t *eps_ptr,
                                   const uint32_t *eps_arc, int64_t E, const int32_t *eps_rank, int num_ranks,
                                   int start,
                                   float beam, float acoustic_scale, int allow_partial, int64_t list_cap,
                                   int64_t log_cap, int word_cap, int threads, float *out_cost,
                                   int32_t *out_reached_final,
                                   int32_t *out_alignment, int32_t *out_num_active, int32_t *out_words,
                                   int32_t *out_num_words, int32_t *out_overflow, void *workspace,
                                   int64_t workspace_bytes, void *stream) {
    if (B < 0 || T < 0 || C < 1 || N < 1 || A < 0 || E < 0 || E > A || num_ranks < 0 || word_cap < 1) return ASR_EINVAL;
    if (threads != 0 && threads != 256 && threads != 512 && threads != 1024) return ASR_EINVAL;
    if (start < 0 || start >= N || !(beam >= 0.f) || !caps_ok(list_cap, log_cap)) return ASR_EINVAL;
    if (frame_stride < (int64_t)B * C) return ASR_EINVAL;
    if (B == 0) return ASR_OK;
    if (!shapes_ok(N, A, C, T)) return ASR_EUNSUPPORTED;
    if (!lp || !lens || !arc_ptr || !final_cost || !eps_ptr || !eps_rank || !out_cost || !out_reached_final ||
        !out_alignment || !out_num_active || !out_words || !out_num_words || !out_overflow)
        return ASR_EINVAL;
    if (A > 0 && (!arc_src || !arc_dst || !arc_ilabel || !arc_olabel || !arc_weight)) return ASR_EINVAL;
    if (E > 0 && !eps_arc) return ASR_EINVAL;
    const Layout l = layout(N, B, list_cap, log_cap);
    if (!workspace || workspace_bytes < l.total) return ASR_EINVAL;
    uint8_t *const ws = (uint8_t *)workspace;
    if (hipMemsetAsync(ws + l.tab, 0xFF, (size_t)B * N * 8, (hipStream_t)stream) != hipSuccess) return ASR_ELAUNCH;
    Params p;
    p.g = Graph{(uint32_t)N, (uint32_t)A, (uint32_t)E, arc_ptr, arc_src, arc_dst, arc_ilabel, arc_olabel, arc_weight, final_cost,
                eps_ptr, eps_arc, eps_rank, num_ranks, (uint32_t)start};
    p.lp = lp;
    p.frame_stride = frame_stride;
    p.lens = lens;
    p.T = T;
    p.B = B;
    p.C = C;
    p.beam = beam;
    p.scale = acoustic_scale;
    p.allow_partial = allow_partial;
    p.list_cap = (uint32_t)list_cap;
    p.log_cap = (uint32_t)log_cap;
    p.word_cap = word_cap;
    p.out_cost = out_cost;
    p.out_final = out_reached_final;
    p.out_align = out_alignment;
    p.out_nact = out_num_active;
    p.out_words = out_words;
    p.out_nwords = out_num_words;
    p.out_overflow = out_overflow;
    p.tab = (unsigned long long *)(ws + l.tab);
    p.slot = (uint32_t *)(ws + l.slot);
    p.lists = (uint32_t *)(ws + l.lists);
    p.rec = (uint32_t *)(ws + l.rec);
    const size_t lds = (size_t)C * sizeof(float);
    switch (pick_threads(B, threads)) {
    case 256: hipLaunchKernelGGL(wfst_decode_kernel<256>, dim3(B), dim3(256), lds, (hipStream_t)stream, p); break;
    case 512: hipLaunchKernelGGL(wfst_decode_kernel<512>, dim3(B), dim3(512), lds, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL(wfst_decode_kernel<1024>, dim3(B), dim3(1024), lds, (hipStream_t)stream, p); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
