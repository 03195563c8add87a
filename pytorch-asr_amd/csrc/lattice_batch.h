// The device lattice batch of the dynamic programmes in lattice_dp.hip, lattice_oracle.hip and lattice_train.hip
// (DESIGN.md section 4.27): its header struct, the checked traversal of its levels, nodes and arcs, the fp64
// arithmetic of an arc and of an end node, and the host validation of the arguments the entry points share.
//
// The lattices are those of asr_wfst_lattice_f32 in the canonical form of DESIGN.md section 4.20, laid end to
// end: nodes by (utterance, time, state), arcs by (utterance, source node, graph arc).  A node's level is (time,
// epsilon rank of its state); every arc rises in level.  The tensors may come from a caller, so a kernel uses a
// node, arc, level or graph index read from memory only after the helper that read it returned true; false
// means: raise the utterance's status word.  The helpers hold no device intrinsic, so a host program can run
// them under a sanitizer (tests/lattice_batch_host.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/asr_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LAT_HD __host__ __device__ __forceinline__
#else
#define LAT_HD inline
#endif

namespace {

constexpr double DINF = __builtin_huge_val();

struct Lat {
    int B;
    int64_t N, A, L, G, S;                  // nodes, arcs, levels of the batch; graph arcs and states
    const int64_t *node_off, *arc_off, *level_off;      // [B + 1]
    const int32_t *time, *state, *level;    // [N]; level: index into level_ptr
    const int32_t *src, *dst;               // [A] node indices of the utterance
    const int64_t *arc;                     // [A] arc index in the graph
    const float *lp;                        // [A] the scores frozen at decode time; null: not read
    const int32_t *level_ptr, *level_node;  // [L + 1], [N]: the nodes of a level (batch indices)
    const int32_t *in_ptr, *in_arc;         // [N + 1], [A]: the in-arcs of a node (batch indices)
    const int32_t *out_ptr;                 // [N + 1]: the out-arcs of node v are [out_ptr[v], out_ptr[v + 1])
    const int32_t *frames, *reached;        // [B]
    const double *own_scale;                // [B] the scale of the search
    const float *w, *fin;                   // graph: [G], [S]
    const int32_t *ol, *il;                 // [G] output labels; input labels (class + 1; 0: epsilon); null: not read
    int start;
    int b_begin, b_count;
    int64_t n_begin, n_end;                 // node_off[b_begin], node_off[b_begin + b_count]: the workspace's nodes
};

// the nodes, arcs and levels of one utterance; ok: inside the batch, and the nodes inside the launch's workspace
struct Span {
    int64_t n0, n1, a0, a1, l0, l1;
    bool ok;
};

LAT_HD Span span_of(const Lat &t, int b) {
    Span s;
    s.n0 = t.node_off[b], s.n1 = t.node_off[b + 1];
    s.a0 = t.arc_off[b], s.a1 = t.arc_off[b + 1];
    s.l0 = t.level_off[b], s.l1 = t.level_off[b + 1];
    s.ok = t.n_begin <= s.n0 && s.n0 <= s.n1 && s.n1 <= t.n_end && s.n1 <= t.N && 0 <= s.a0 && s.a0 <= s.a1 &&
           s.a1 <= t.A && 0 <= s.l0 && s.l0 <= s.l1 && s.l1 <= t.L;
    return s;
}

// ---- checked traversal: sp.ok first, then levels_cover, then level by level ----------------------------------
// the utterance's levels hold exactly its nodes
LAT_HD bool levels_cover(const Lat &t, const Span &sp) {
    return t.level_ptr[sp.l0] == sp.n0 && t.level_ptr[sp.l1] == sp.n1;
}

// [e0, e1) = [level_ptr[l], level_ptr[l + 1]), the positions of level l in level_node, against the utterance's
// nodes [n0, n1).  The sweep reads the two words itself (l is inside [sp.l0, sp.l1), so the read is safe) and
// passes scalars: with the loads in here lattice_seqtrain_kernel loses a wave of occupancy, with sp passed by
// reference lattice_bestpath_kernel keeps it in scratch (DESIGN.md section 4.27 has the figures).
LAT_HD bool level_range(int64_t e0, int64_t e1, int64_t n0, int64_t n1) { return e0 >= n0 && e0 <= e1 && e1 <= n1; }

// the node v at position e of level l
LAT_HD bool node_at(const Lat &t, const Span &sp, int64_t e, int64_t l, int64_t &v) {
    v = t.level_node[e];
    return v >= sp.n0 && v < sp.n1 && t.level[v] == l;
}

// the positions [j0, j1) of node v's in-arcs in in_arc; its out-arcs [j0, j1) themselves
LAT_HD bool in_arcs_of(const Lat &t, const Span &sp, int64_t v, int64_t &j0, int64_t &j1) {
    j0 = t.in_ptr[v], j1 = t.in_ptr[v + 1];
    return j0 >= sp.a0 && j0 <= j1 && j1 <= sp.a1;
}

LAT_HD bool out_arcs_of(const Lat &t, const Span &sp, int64_t v, int64_t &j0, int64_t &j1) {
    j0 = t.out_ptr[v], j1 = t.out_ptr[v + 1];
    return j0 >= sp.a0 && j0 <= j1 && j1 <= sp.a1;
}

// the in-arc a at position j of node v of level l, its source u and graph arc g
LAT_HD bool in_arc_at(const Lat &t, const Span &sp, int64_t j, int64_t v, int64_t l, int64_t &a, int64_t &u,
                      int64_t &g) {
    a = t.in_arc[j];
    if (a < sp.a0 || a >= sp.a1) return false;
    u = sp.n0 + t.src[a], g = t.arc[a];
    if (sp.n0 + t.dst[a] != v || u < sp.n0 || u >= sp.n1 || g < 0 || g >= t.G) return false;
    const int32_t lu = t.level[u];
    return lu >= sp.l0 && lu < l;               // the level must rise: u is final in an upward sweep
}

// the out-arc a (inside out_arcs_of) of node v of level l, its destination d and graph arc g
LAT_HD bool out_arc_at(const Lat &t, const Span &sp, int64_t a, int64_t v, int64_t l, int64_t &d, int64_t &g) {
    d = sp.n0 + t.dst[a], g = t.arc[a];
    if (sp.n0 + t.src[a] != v || d < sp.n0 || d >= sp.n1 || g < 0 || g >= t.G) return false;
    const int32_t ld = t.level[d];
    return ld > l && ld < sp.l1;                // the level must rise: d is final in a downward sweep
}

// arc a of [sp.a0, sp.a1) on its own, whatever node ranges cover it: both ends and the graph arc
LAT_HD bool arc_at(const Lat &t, const Span &sp, int64_t a, int64_t &u, int64_t &d, int64_t &g) {
    u = sp.n0 + t.src[a], d = sp.n0 + t.dst[a], g = t.arc[a];
    return u >= sp.n0 && u < sp.n1 && d >= sp.n0 && d < sp.n1 && g >= 0 && g < t.G;
}

// the arc a = sp.a0 + back (back >= 0) that a back-pointer of node cur names, its source u and graph arc g
LAT_HD bool back_arc_at(const Lat &t, const Span &sp, int32_t back, int64_t cur, int64_t &a, int64_t &u,
                        int64_t &g) {
    a = sp.a0 + back;
    if (a >= sp.a1) return false;
    g = t.arc[a], u = sp.n0 + t.src[a];
    return g >= 0 && g < t.G && u >= sp.n0 && u < sp.n1 && t.level[u] < t.level[cur];
}

// ---- arithmetic: fp64, every step one rounding --------------------------------------------------------------
// the acoustic scale of utterance b: NaN asks for the scale of its search
LAT_HD double scale_of(const Lat &t, int b, double ac_scale) {
    return ac_scale != ac_scale ? t.own_scale[b] : ac_scale;
}

// x = fl(fl(lm w) - fl(sc lp)).  The pragma keeps it from being contracted to an fma under hipcc's default
// (-ffp-contract=fast-honor-pragmas) and under -ffp-contract=on; an explicit -ffp-contract=fast overrides it,
// so the Makefile builds every includer with -ffp-contract=off as well.
LAT_HD double arc_cost(double lm, double sc, float w, float lp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = lm * (double)w;
    const double b = sc * (double)lp;
    return a - b;
}

// the unscaled cost of stopping at node v (+inf: not an end node); 0 at the last time of a partial lattice
LAT_HD double end_cost(const Lat &t, int64_t v, int frames, int reached, bool &bad) {
    if (t.time[v] != frames) return DINF;
    if (!reached) return 0.0;
    const int s = t.state[v];
    if (s < 0 || s >= t.S) {
        bad = true;
        return DINF;
    }
    return (double)t.fin[s];
}

// fl(lm end(v)) as Lattice._end_costs has it
LAT_HD double scaled_end(const Lat &t, int64_t v, int frames, int reached, double lm, bool &bad) {
    if (t.time[v] != frames) return DINF;
    if (!reached) return 0.0;
    const int s = t.state[v];
    if (s < 0 || s >= t.S) {
        bad = true;
        return DINF;
    }
    return lm * (double)t.fin[s];
}

LAT_HD double lse_value(double m, double s) { return m == -DINF ? -DINF : m + log(s); }

// a - x for log weights: -inf as soon as the path weight is zero
LAT_HD double log_times(double a, double x) { return (a == -DINF || x == DINF) ? -DINF : a - x; }

// ---- host side ----------------------------------------------------------------------------------------------
inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

inline bool sizes_ok(int64_t N, int64_t A, int64_t L) {
    const int64_t lim = ((int64_t)1 << 31) - 1;
    return N >= 0 && A >= 0 && L >= 0 && N < lim && A < lim && L < lim;
}

// the host copies of the offsets: [B + 1], from 0 to total, never decreasing
inline bool offsets_ok(const int64_t *h, int B, int64_t total) {
    if (!h || h[0] != 0 || h[B] != total) return false;
    for (int b = 0; b < B; ++b)
        if (h[b + 1] < h[b]) return false;
    return true;
}

inline bool threads_ok(int threads) { return threads == 0 || threads == 64 || threads == 128 || threads == 256; }

// the per-arc arrays an operation reads besides the batch's own: fill_lat wants them non-null when there are arcs
enum { LAT_LP = 1, LAT_OLABEL = 2, LAT_ILABEL = 4 };

// Validates what every lattice entry point takes and fills t.  In this order: ASR_EINVAL for bad counts,
// ASR_EUNSUPPORTED for sizes, ASR_EINVAL for the host offsets and for null pointers.
inline int fill_lat(Lat &t, int needs, int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L,
                    const int64_t *h_node_off, const int64_t *h_arc_off, const int64_t *h_level_off,
                    const int64_t *node_off, const int64_t *arc_off, const int64_t *level_off,
                    const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
                    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
                    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
                    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final,
                    const double *own_scale, int64_t S, int64_t G, const float *arc_weight, const int32_t *arc_olabel,
                    const int32_t *arc_ilabel, const float *final_cost, int start) {
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
    if (A > 0 && (!lat_src || !lat_dst || !lat_arc || !in_arc || !arc_weight)) return ASR_EINVAL;
    if (A > 0 && (((needs & LAT_LP) && !lat_lp) || ((needs & LAT_OLABEL) && !arc_olabel) ||
                  ((needs & LAT_ILABEL) && !arc_ilabel)))
        return ASR_EINVAL;
    t = Lat{B, N, A, L, G, S, node_off, arc_off, level_off, node_time, node_state, node_level, lat_src, lat_dst,
            lat_arc, (needs & LAT_LP) ? lat_lp : nullptr, level_ptr, level_node, in_ptr, in_arc, out_ptr, num_frames,
            reached_final, own_scale, arc_weight, final_cost, (needs & LAT_OLABEL) ? arc_olabel : nullptr,
            (needs & LAT_ILABEL) ? arc_ilabel : nullptr, start, b_begin, b_count, h_node_off[b_begin],
            h_node_off[b_begin + b_count]};
    return ASR_OK;
}

#if defined(__HIPCC__)
// One workgroup of `threads` lanes (0: dflt) per block of the grid, from the kernel's three instantiations.
template <typename Args>
int launch_by_threads(int threads, int dflt, int64_t blocks, void *stream, const Args &q, void (*k64)(Args),
                      void (*k128)(Args), void (*k256)(Args)) {
    const int nt = threads ? threads : dflt;
    void (*const kernel)(Args) = nt == 256 ? k256 : nt == 128 ? k128 : k64;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)nt), 0, (hipStream_t)stream, q);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
#endif

}  // namespace
