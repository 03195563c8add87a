// csrc/lattice_batch.h on the host, under AddressSanitizer and UBSan (tests/test_lattice_batch_host.py builds and
// runs this program; it needs no GPU).  A batch of two utterances, 6 nodes, 8 arcs and 5 levels lives in heap
// arrays of exactly the batch's sizes, so a read past any end is a sanitizer report.  The traversal helpers must
// visit every node and arc once, and after every single corruption the named helper must return false before
// the bad index is used.  fill_lat is run over a table of argument sets with the codes its order of checks gives.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

#include "../pytorch-asr_amd/csrc/lattice_batch.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T> &v) {   // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

constexpr float FINF = __builtin_huge_valf();

// utterance 0: nodes 0..3 on levels {0}, {1, 2}, {3}; arcs 0>1 0>2 0>3 1>3 2>3.  utterance 1: nodes 4, 5 on levels
// {4}, {5}; three parallel arcs 0>1.  src / dst are node indices of the utterance, everything else batch indices.
struct Batch {
    static constexpr int B = 2;
    static constexpr int64_t N = 6, A = 8, L = 5, G = 5, S = 3;
    std::unique_ptr<int64_t[]> node_off = exact<int64_t>({0, 4, 6}), arc_off = exact<int64_t>({0, 5, 8}),
                               level_off = exact<int64_t>({0, 3, 5}), arc = exact<int64_t>({0, 1, 2, 3, 4, 0, 1, 2});
    std::unique_ptr<int32_t[]> time = exact<int32_t>({0, 1, 1, 2, 0, 1}), state = exact<int32_t>({0, 1, 2, 1, 0, 1}),
                               level = exact<int32_t>({0, 1, 1, 2, 3, 4}),
                               src = exact<int32_t>({0, 0, 0, 1, 2, 0, 0, 0}),
                               dst = exact<int32_t>({1, 2, 3, 3, 3, 1, 1, 1}),
                               level_ptr = exact<int32_t>({0, 1, 3, 4, 5, 6}),
                               level_node = exact<int32_t>({0, 1, 2, 3, 4, 5}),
                               in_ptr = exact<int32_t>({0, 0, 1, 2, 5, 5, 8}),
                               in_arc = exact<int32_t>({0, 1, 2, 3, 4, 5, 6, 7}),
                               out_ptr = exact<int32_t>({0, 3, 4, 5, 5, 8, 8}), frames = exact<int32_t>({2, 1}),
                               reached = exact<int32_t>({1, 1}), ol = exact<int32_t>({0, 7, 8, 0, 9}),
                               il = exact<int32_t>({1, 2, 0, 1, 2});
    std::unique_ptr<float[]> lp = exact<float>({-1, -2, -3, -4, -5, -6, -7, -8}),
                             w = exact<float>({0.5f, 1.5f, 2.5f, 3.5f, 4.5f}), fin = exact<float>({FINF, 0.5f, 1.0f});
    std::unique_ptr<double[]> own_scale = exact<double>({1.0, 0.25});

    Lat lat() const {               // one launch over both utterances
        return Lat{B, N, A, L, G, S, node_off.get(), arc_off.get(), level_off.get(), time.get(), state.get(),
                   level.get(), src.get(), dst.get(), arc.get(), lp.get(), level_ptr.get(), level_node.get(),
                   in_ptr.get(), in_arc.get(), out_ptr.get(), frames.get(), reached.get(), own_scale.get(), w.get(),
                   fin.get(), ol.get(), il.get(), 0, 0, B, 0, N};
    }
};

enum Step { DONE, SPAN, COVER, LEVEL_RANGE, NODE_AT, IN_ARCS_OF, IN_ARC_AT, OUT_ARCS_OF, OUT_ARC_AT, ARC_AT, END_COST };
const char *const STEP_NAME[] = {"done", "span_of", "levels_cover", "level_range", "node_at", "in_arcs_of", "in_arc_at",
                                 "out_arcs_of", "out_arc_at", "arc_at", "end_cost"};
enum Sweep { UP = 1, DOWN = 2, ARCS = 4, ENDS = 8, ALL = 15 };

// The sweeps of the kernels over utterance b, an index used only after its helper returned true.  Returns the
// first helper that refused, and counts the visits of every node, in-arc and out-arc.
Step walk(const Lat &t, int b, int sweeps, std::vector<int> &nodes, std::vector<int> &ins, std::vector<int> &outs) {
    const Span sp = span_of(t, b);
    if (!sp.ok) return SPAN;
    if (!levels_cover(t, sp)) return COVER;
    if (sweeps & UP) {
        for (int64_t l = sp.l0; l < sp.l1; ++l) {
            const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
            if (!level_range(e0, e1, sp.n0, sp.n1)) return LEVEL_RANGE;
            for (int64_t e = e0; e < e1; ++e) {
                int64_t v, j0, j1;
                if (!node_at(t, sp, e, l, v)) return NODE_AT;
                ++nodes[v];
                if (!in_arcs_of(t, sp, v, j0, j1)) return IN_ARCS_OF;
                for (int64_t j = j0; j < j1; ++j) {
                    int64_t a, u, g;
                    if (!in_arc_at(t, sp, j, v, l, a, u, g)) return IN_ARC_AT;
                    ++ins[a];
                    CHECK(u == sp.n0 + t.src[a] && g == t.arc[a] && t.level[u] < l);
                    (void)(t.w[g] + t.lp[a] + (float)t.ol[g] + (float)t.il[g]);    // what a kernel reads next
                }
            }
        }
    }
    if (sweeps & DOWN) {            // the levels and their nodes were checked going up, as in the kernels
        for (int64_t l = sp.l1 - 1; l >= sp.l0; --l) {
            const int64_t e0 = t.level_ptr[l], e1 = t.level_ptr[l + 1];
            if (!level_range(e0, e1, sp.n0, sp.n1)) return LEVEL_RANGE;
            for (int64_t e = e0; e < e1; ++e) {
                int64_t v, j0, j1;
                if (!node_at(t, sp, e, l, v)) return NODE_AT;
                if (!out_arcs_of(t, sp, v, j0, j1)) return OUT_ARCS_OF;
                for (int64_t a = j0; a < j1; ++a) {
                    int64_t d, g;
                    if (!out_arc_at(t, sp, a, v, l, d, g)) return OUT_ARC_AT;
                    ++outs[a];
                    CHECK(d == sp.n0 + t.dst[a] && g == t.arc[a] && t.level[d] > l);
                    (void)(t.w[g] + t.lp[a]);
                }
            }
        }
    }
    if (sweeps & ARCS) {
        for (int64_t a = sp.a0; a < sp.a1; ++a) {
            int64_t u, d, g;
            if (!arc_at(t, sp, a, u, d, g)) return ARC_AT;
            (void)(t.time[u] + t.time[d] + (int32_t)t.w[g]);
        }
    }
    if (sweeps & ENDS) {
        for (int64_t v = sp.n0; v < sp.n1; ++v) {
            bool bad = false;
            (void)end_cost(t, v, t.frames[b], t.reached[b], bad);
            bool bad2 = false;
            (void)scaled_end(t, v, t.frames[b], t.reached[b], 2.0, bad2);
            CHECK(bad == bad2);
            if (bad) return END_COST;
        }
    }
    return DONE;
}

Step walk(const Lat &t, int b, int sweeps) {
    std::vector<int> nodes(Batch::N), ins(Batch::A), outs(Batch::A);
    return walk(t, b, sweeps, nodes, ins, outs);
}

void test_full_traversal() {
    const Batch h;
    const Lat t = h.lat();
    std::vector<int> nodes(Batch::N), ins(Batch::A), outs(Batch::A);
    for (int b = 0; b < Batch::B; ++b) CHECK(walk(t, b, ALL, nodes, ins, outs) == DONE);
    for (int v = 0; v < Batch::N; ++v) CHECK(nodes[v] == 1);
    for (int a = 0; a < Batch::A; ++a) CHECK(ins[a] == 1 && outs[a] == 1);
    // a launch over utterance 1 alone: its workspace starts at node 4, and utterance 0 lies before it
    Lat one = t;
    one.b_begin = 1, one.b_count = 1, one.n_begin = 4, one.n_end = 6;
    CHECK(walk(one, 1, ALL) == DONE);
    CHECK(walk(one, 0, ALL) == SPAN);
}

struct Corruption {
    const char *what;
    std::function<void(Batch &, Lat &)> apply;
    int b, sweeps;
    Step want;
};

void test_corruptions() {
    const int32_t BIG = 1000000;
    const std::vector<Corruption> table = {
        {"node_off beyond the batch", [&](Batch &h, Lat &) { h.node_off[2] = BIG; }, 1, ALL, SPAN},
        {"node_off before the launch", [&](Batch &h, Lat &) { h.node_off[0] = -1; }, 0, ALL, SPAN},
        {"node_off decreasing", [&](Batch &h, Lat &) { h.node_off[1] = 7; }, 1, ALL, SPAN},
        {"arc_off beyond the batch", [&](Batch &h, Lat &) { h.arc_off[1] = BIG; }, 0, ALL, SPAN},
        {"arc_off negative", [&](Batch &h, Lat &) { h.arc_off[0] = -1; }, 0, ALL, SPAN},
        {"level_off beyond the batch", [&](Batch &h, Lat &) { h.level_off[2] = BIG; }, 1, ALL, SPAN},
        {"level_off negative", [&](Batch &h, Lat &) { h.level_off[0] = -3; }, 0, ALL, SPAN},
        {"n1 beyond the launch's nodes", [&](Batch &, Lat &t) { t.b_count = 1, t.n_end = 4; }, 1, ALL, SPAN},
        {"level_ptr: first level elsewhere", [&](Batch &h, Lat &) { h.level_ptr[0] = 1; }, 0, ALL, COVER},
        {"level_ptr: last level elsewhere", [&](Batch &h, Lat &) { h.level_ptr[5] = 5; }, 1, ALL, COVER},
        {"level_ptr beyond the nodes", [&](Batch &h, Lat &) { h.level_ptr[1] = BIG; }, 0, ALL, LEVEL_RANGE},
        {"level_ptr negative", [&](Batch &h, Lat &) { h.level_ptr[1] = -1; }, 0, ALL, LEVEL_RANGE},
        {"level_ptr decreasing", [&](Batch &h, Lat &) { h.level_ptr[2] = 0; }, 0, ALL, LEVEL_RANGE},
        {"level_node beyond the nodes", [&](Batch &h, Lat &) { h.level_node[1] = BIG; }, 0, ALL, NODE_AT},
        {"level_node negative", [&](Batch &h, Lat &) { h.level_node[1] = -1; }, 0, ALL, NODE_AT},
        {"level_node of the other utterance", [&](Batch &h, Lat &) { h.level_node[4] = 3; }, 1, ALL, NODE_AT},
        {"node_level beyond the levels", [&](Batch &h, Lat &) { h.level[0] = BIG; }, 0, ALL, NODE_AT},
        {"node_level negative", [&](Batch &h, Lat &) { h.level[2] = -1; }, 0, ALL, NODE_AT},
        {"in_ptr beyond the arcs", [&](Batch &h, Lat &) { h.in_ptr[2] = BIG; }, 0, ALL, IN_ARCS_OF},
        {"in_ptr negative", [&](Batch &h, Lat &) { h.in_ptr[1] = -1; }, 0, ALL, IN_ARCS_OF},
        {"in_ptr into the other utterance", [&](Batch &h, Lat &) { h.in_ptr[4] = 6; }, 0, ALL, IN_ARCS_OF},
        {"in_arc beyond the arcs", [&](Batch &h, Lat &) { h.in_arc[1] = BIG; }, 0, ALL, IN_ARC_AT},
        {"in_arc negative", [&](Batch &h, Lat &) { h.in_arc[5] = -1; }, 1, ALL, IN_ARC_AT},
        {"in_arc of another node", [&](Batch &h, Lat &) { h.in_arc[0] = 1; }, 0, ALL, IN_ARC_AT},
        {"src beyond the nodes", [&](Batch &h, Lat &) { h.src[3] = BIG; }, 0, UP, IN_ARC_AT},
        {"src negative", [&](Batch &h, Lat &) { h.src[3] = -1; }, 0, UP, IN_ARC_AT},
        {"dst beyond the nodes", [&](Batch &h, Lat &) { h.dst[3] = BIG; }, 0, UP, IN_ARC_AT},
        {"arc beyond the graph", [&](Batch &h, Lat &) { h.arc[1] = BIG; }, 0, UP, IN_ARC_AT},
        {"arc negative", [&](Batch &h, Lat &) { h.arc[6] = -1; }, 1, UP, IN_ARC_AT},
        {"an in-arc whose level does not rise", [&](Batch &h, Lat &) { h.src[4] = 3; }, 0, UP, IN_ARC_AT},
        {"out_ptr beyond the arcs", [&](Batch &h, Lat &) { h.out_ptr[2] = BIG; }, 0, DOWN, OUT_ARCS_OF},
        {"out_ptr negative", [&](Batch &h, Lat &) { h.out_ptr[0] = -1; }, 0, DOWN, OUT_ARCS_OF},
        {"src beyond the nodes, going down", [&](Batch &h, Lat &) { h.src[3] = BIG; }, 0, DOWN, OUT_ARC_AT},
        {"dst beyond the nodes, going down", [&](Batch &h, Lat &) { h.dst[3] = BIG; }, 0, DOWN, OUT_ARC_AT},
        {"dst negative, going down", [&](Batch &h, Lat &) { h.dst[6] = -7; }, 1, DOWN, OUT_ARC_AT},
        {"arc beyond the graph, going down", [&](Batch &h, Lat &) { h.arc[1] = BIG; }, 0, DOWN, OUT_ARC_AT},
        {"an out-arc whose level does not rise", [&](Batch &h, Lat &) { h.dst[3] = 1; }, 0, DOWN, OUT_ARC_AT},
        {"src beyond the nodes, arc by arc", [&](Batch &h, Lat &) { h.src[2] = BIG; }, 0, ARCS, ARC_AT},
        {"dst negative, arc by arc", [&](Batch &h, Lat &) { h.dst[7] = -1; }, 1, ARCS, ARC_AT},
        {"arc beyond the graph, arc by arc", [&](Batch &h, Lat &) { h.arc[4] = Batch::G; }, 0, ARCS, ARC_AT},
        {"state beyond the graph", [&](Batch &h, Lat &) { h.state[3] = BIG; }, 0, ENDS, END_COST},
        {"state negative", [&](Batch &h, Lat &) { h.state[5] = -1; }, 1, ENDS, END_COST},
    };
    for (const Corruption &c : table) {
        Batch h;
        Lat t = h.lat();
        c.apply(h, t);
        const Step got = walk(t, c.b, c.sweeps);
        if (got != c.want) {
            std::printf("FAILED %s: %s refused, expected %s\n", c.what, STEP_NAME[got], STEP_NAME[c.want]);
            ++failures;
        }
    }
}

void test_back_arc() {
    const Batch h;
    const Lat t = h.lat();
    const Span sp = span_of(t, 0);
    int64_t a, u, g;
    CHECK(back_arc_at(t, sp, 3, 3, a, u, g) && a == 3 && u == 1 && g == 3);      // arc 1 > 3 from node 3
    CHECK(!back_arc_at(t, sp, 7, 3, a, u, g));                                   // an arc of the other utterance
    CHECK(!back_arc_at(t, sp, 3, 1, a, u, g));                                   // its source is not below node 1
    Batch bad;
    bad.src[3] = 1000000;
    CHECK(!back_arc_at(bad.lat(), sp, 3, 3, a, u, g));
    bad.src[3] = 1, bad.arc[3] = -1;
    CHECK(!back_arc_at(bad.lat(), sp, 3, 3, a, u, g));
}

void test_arithmetic() {
    const Batch h;
    const Lat t = h.lat();
    bool bad = false;
    CHECK(end_cost(t, 3, 2, 1, bad) == 0.5 && scaled_end(t, 3, 2, 1, 3.0, bad) == 1.5 && !bad);
    CHECK(end_cost(t, 1, 2, 1, bad) == DINF && scaled_end(t, 1, 2, 1, 3.0, bad) == DINF);   // not at the last frame
    CHECK(end_cost(t, 3, 2, 0, bad) == 0.0 && scaled_end(t, 3, 2, 0, 3.0, bad) == 0.0);     // a partial lattice
    CHECK(end_cost(t, 4, 0, 1, bad) == DINF && !bad);                                       // state 0 is not final
    CHECK(scale_of(t, 1, 2.0) == 2.0 && scale_of(t, 1, __builtin_nan("")) == 0.25);
    // fl(fl(lm w) - fl(sc lp)): lm w = 1 + 2^-23 + 2^-30 + 2^-53 rounds to sc lp, so the difference is 0; an fma
    // would keep the 2^-53.  The operands are volatile, so the compiler does the arithmetic at run time.  This can
    // fail only in a build that may emit fma (the driver adds -mfma -ffp-contract=fast-honor-pragmas where the CPU
    // and the compiler have them); in a baseline x86-64 build it states the rule without pinning it.
    volatile double lm = 1.0 + 0x1p-30, sc = 1.0 + 0x1p-23 + 0x1p-30;
    volatile float w = 1.0f + 0x1p-23f, lp = 1.0f;
    CHECK(arc_cost(lm, sc, w, lp) == 0.0);
    CHECK(arc_cost(2.0, 0.5, 3.0f, -4.0f) == 8.0);
    CHECK(lse_value(-DINF, 0.0) == -DINF && lse_value(1.0, 1.0) == 1.0);
    CHECK(log_times(-DINF, 1.0) == -DINF && log_times(1.0, DINF) == -DINF && log_times(1.0, -DINF) == DINF);
    CHECK(log_times(3.0, 1.0) == 2.0);
    CHECK(up16(0) == 0 && up16(1) == 16 && up16(16) == 16 && up16(17) == 32);
    CHECK(threads_ok(0) && threads_ok(64) && threads_ok(128) && threads_ok(256) && !threads_ok(32) && !threads_ok(512));
}

// what every lattice entry point passes to fill_lat; the device pointers are only tested against null
struct Args {
    int needs = LAT_LP | LAT_OLABEL, B = 2, b_begin = 0, b_count = 2;
    int64_t N = 6, A = 8, L = 5, S = 3, G = 5;
    int start = 0;
    std::vector<int64_t> hn = {0, 4, 6}, ha = {0, 5, 8}, hl = {0, 3, 5};
    const int64_t *h_node_off = hn.data(), *h_arc_off = ha.data(), *h_level_off = hl.data();
    int64_t i64 = 0;
    int32_t i32 = 0;
    float f32 = 0;
    double f64 = 0;
    const int64_t *node_off = &i64, *arc_off = &i64, *level_off = &i64, *lat_arc = &i64;
    const int32_t *node_time = &i32, *node_state = &i32, *node_level = &i32, *lat_src = &i32, *lat_dst = &i32,
                  *level_ptr = &i32, *level_node = &i32, *in_ptr = &i32, *in_arc = &i32, *out_ptr = &i32,
                  *num_frames = &i32, *reached_final = &i32, *arc_olabel = &i32, *arc_ilabel = &i32;
    const float *lat_lp = &f32, *arc_weight = &f32, *final_cost = &f32;
    const double *own_scale = &f64;

    void shape(int B_, int64_t N_, int64_t A_, int64_t L_) {     // one utterance with everything, the rest empty
        B = B_, b_count = B_, N = N_, A = A_, L = L_;
        hn.assign(B_ + 1, N_), ha.assign(B_ + 1, A_), hl.assign(B_ + 1, L_);
        hn[0] = ha[0] = hl[0] = 0;
        h_node_off = hn.data(), h_arc_off = ha.data(), h_level_off = hl.data();
    }
    int call(Lat &t) const {
        return fill_lat(t, needs, B, b_begin, b_count, N, A, L, h_node_off, h_arc_off, h_level_off, node_off, arc_off,
                        level_off, node_time, node_state, node_level, lat_src, lat_dst, lat_arc, lat_lp, level_ptr,
                        level_node, in_ptr, in_arc, out_ptr, num_frames, reached_final, own_scale, S, G, arc_weight,
                        arc_olabel, arc_ilabel, final_cost, start);
    }
};

void expect(const char *what, int want, const std::function<void(Args &)> &change) {
    Args a;
    change(a);
    Lat t;
    const int got = a.call(t);
    if (got != want) {
        std::printf("FAILED fill_lat, %s: returned %d, expected %d\n", what, got, want);
        ++failures;
    }
}

void test_fill_lat() {
    const int64_t TOP = ((int64_t)1 << 31) - 1;
    {
        Args a;
        Lat t;
        CHECK(a.call(t) == ASR_OK);
        CHECK(t.B == 2 && t.N == 6 && t.A == 8 && t.L == 5 && t.G == 5 && t.S == 3 && t.n_begin == 0 && t.n_end == 6);
        CHECK(t.lp == a.lat_lp && t.ol == a.arc_olabel && t.il == nullptr && t.out_ptr == a.out_ptr);
        a.b_begin = 1, a.b_count = 1, a.needs = LAT_ILABEL, a.lat_lp = nullptr, a.arc_olabel = nullptr;
        CHECK(a.call(t) == ASR_OK);
        CHECK(t.n_begin == 4 && t.n_end == 6 && t.b_begin == 1 && t.b_count == 1);
        CHECK(t.lp == nullptr && t.ol == nullptr && t.il == a.arc_ilabel);
    }
    // bad counts: ASR_EINVAL, before the sizes are looked at
    expect("B < 0", ASR_EINVAL, [](Args &a) { a.B = -1; });
    expect("b_begin < 0", ASR_EINVAL, [](Args &a) { a.b_begin = -1; });
    expect("b_count < 0", ASR_EINVAL, [](Args &a) { a.b_count = -1; });
    expect("b_begin + b_count > B", ASR_EINVAL, [](Args &a) { a.b_begin = 1; });
    expect("b_begin + b_count overflows int", ASR_EINVAL, [](Args &a) { a.b_begin = 0x7fffffff; });
    expect("N < 0", ASR_EINVAL, [](Args &a) { a.N = -1; });
    expect("A < 0", ASR_EINVAL, [](Args &a) { a.A = -1; });
    expect("L < 0", ASR_EINVAL, [](Args &a) { a.L = -1; });
    expect("no states", ASR_EINVAL, [](Args &a) { a.S = 0; });
    expect("G < 0", ASR_EINVAL, [](Args &a) { a.G = -1; });
    expect("start < 0", ASR_EINVAL, [](Args &a) { a.start = -1; });
    expect("start beyond the states", ASR_EINVAL, [](Args &a) { a.start = 3; });
    expect("B < 0 and N too large", ASR_EINVAL, [&](Args &a) { a.B = -1, a.N = TOP; });
    // sizes: ASR_EUNSUPPORTED, before the offsets and the pointers
    expect("N at 2^31 - 1", ASR_EUNSUPPORTED, [&](Args &a) { a.N = TOP; });
    expect("A at 2^31 - 1", ASR_EUNSUPPORTED, [&](Args &a) { a.A = TOP; });
    expect("L at 2^31 - 1", ASR_EUNSUPPORTED, [&](Args &a) { a.L = TOP; });
    expect("N too large and no host offsets", ASR_EUNSUPPORTED, [&](Args &a) { a.N = TOP, a.h_node_off = nullptr; });
    expect("A too large and a null pointer", ASR_EUNSUPPORTED, [&](Args &a) { a.A = TOP + 5, a.in_ptr = nullptr; });
    expect("N just below the limit, offsets of another size", ASR_EINVAL, [&](Args &a) { a.N = TOP - 1; });
    // the host offsets
    expect("no host node offsets", ASR_EINVAL, [](Args &a) { a.h_node_off = nullptr; });
    expect("no host arc offsets", ASR_EINVAL, [](Args &a) { a.h_arc_off = nullptr; });
    expect("no host level offsets", ASR_EINVAL, [](Args &a) { a.h_level_off = nullptr; });
    expect("offsets not from 0", ASR_EINVAL, [](Args &a) { a.hn[0] = 1; });
    expect("offsets not up to N", ASR_EINVAL, [](Args &a) { a.hn[2] = 5; });
    expect("offsets not up to A", ASR_EINVAL, [](Args &a) { a.A = 9; });
    expect("offsets decreasing", ASR_EINVAL, [](Args &a) { a.hl[1] = 6; });
    expect("more levels than nodes", ASR_EINVAL, [](Args &a) { a.shape(1, 1, 0, 2); });
    expect("more levels than nodes in one utterance", ASR_EINVAL, [](Args &a) { a.hn[1] = 2; });
    expect("nodes without a level", ASR_EINVAL, [](Args &a) { a.shape(1, 1, 0, 0); });
    expect("arcs on one level", ASR_EINVAL, [](Args &a) { a.shape(1, 2, 1, 1); });
    expect("two nodes, an arc, two levels", ASR_OK, [](Args &a) { a.shape(1, 2, 1, 2); });
    // the pointers, each on its own
    expect("node_off", ASR_EINVAL, [](Args &a) { a.node_off = nullptr; });
    expect("arc_off", ASR_EINVAL, [](Args &a) { a.arc_off = nullptr; });
    expect("level_off", ASR_EINVAL, [](Args &a) { a.level_off = nullptr; });
    expect("level_ptr", ASR_EINVAL, [](Args &a) { a.level_ptr = nullptr; });
    expect("in_ptr", ASR_EINVAL, [](Args &a) { a.in_ptr = nullptr; });
    expect("out_ptr", ASR_EINVAL, [](Args &a) { a.out_ptr = nullptr; });
    expect("num_frames", ASR_EINVAL, [](Args &a) { a.num_frames = nullptr; });
    expect("reached_final", ASR_EINVAL, [](Args &a) { a.reached_final = nullptr; });
    expect("own_scale", ASR_EINVAL, [](Args &a) { a.own_scale = nullptr; });
    expect("final_cost", ASR_EINVAL, [](Args &a) { a.final_cost = nullptr; });
    expect("node_time", ASR_EINVAL, [](Args &a) { a.node_time = nullptr; });
    expect("node_state", ASR_EINVAL, [](Args &a) { a.node_state = nullptr; });
    expect("node_level", ASR_EINVAL, [](Args &a) { a.node_level = nullptr; });
    expect("level_node", ASR_EINVAL, [](Args &a) { a.level_node = nullptr; });
    expect("lat_src", ASR_EINVAL, [](Args &a) { a.lat_src = nullptr; });
    expect("lat_dst", ASR_EINVAL, [](Args &a) { a.lat_dst = nullptr; });
    expect("lat_arc", ASR_EINVAL, [](Args &a) { a.lat_arc = nullptr; });
    expect("in_arc", ASR_EINVAL, [](Args &a) { a.in_arc = nullptr; });
    expect("arc_weight", ASR_EINVAL, [](Args &a) { a.arc_weight = nullptr; });
    expect("lat_lp where it is read", ASR_EINVAL, [](Args &a) { a.lat_lp = nullptr; });
    expect("arc_olabel where it is read", ASR_EINVAL, [](Args &a) { a.arc_olabel = nullptr; });
    expect("arc_ilabel where it is not read", ASR_OK, [](Args &a) { a.arc_ilabel = nullptr; });
    expect("arc_ilabel where it is read", ASR_EINVAL, [](Args &a) { a.needs = LAT_ILABEL, a.arc_ilabel = nullptr; });
    expect("lat_lp and arc_olabel where they are not read", ASR_OK,
           [](Args &a) { a.needs = LAT_ILABEL, a.lat_lp = nullptr, a.arc_olabel = nullptr; });
    // no arcs: their arrays may be missing; no nodes: theirs too
    expect("no arcs, no arc arrays", ASR_OK, [](Args &a) {
        a.shape(1, 2, 0, 2);
        a.lat_src = a.lat_dst = a.in_arc = a.arc_olabel = nullptr;
        a.lat_arc = nullptr, a.lat_lp = a.arc_weight = nullptr;
    });
    expect("an empty batch", ASR_OK, [](Args &a) {
        a.shape(1, 0, 0, 0);
        a.node_time = a.node_state = a.node_level = a.level_node = a.lat_src = nullptr;
    });
    expect("an empty batch still needs in_ptr", ASR_EINVAL, [](Args &a) { a.shape(1, 0, 0, 0), a.in_ptr = nullptr; });
    expect("no utterances", ASR_OK, [](Args &a) { a.shape(0, 0, 0, 0); });
}

}  // namespace

int main() {
    test_full_traversal();
    test_corruptions();
    test_back_arc();
    test_arithmetic();
    test_fill_lat();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("lattice_batch_host ok\n");
    return 0;
}
