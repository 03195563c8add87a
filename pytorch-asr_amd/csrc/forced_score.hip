// Forced scoring of given sentences through their prefix trie (the teacher-forced pass of the
// reference's egs/wsj/local/lattice_search/rescore_lattices2.py / score_groundtruth.py):
//
//  asr_forced_level_f32 — the bookkeeping of ONE trie level, the forced counterpart of the beam
//      step kernels: one workgroup per unit slot (a distinct prefix of this length).  It adds this
//      step's alignment to the coverage row of the unit it extends, takes the log-partition of
//      the slot's logits once, and hands log_softmax(logits)[label] along every outgoing edge: to
//      the fp64 running sum of the unit the edge creates, or, on an EOS edge, to the sentence the
//      edge completes, together with the number of covered frames.
//
// A row-wise kernel like softmax.hip / the per-hypothesis part of beam_lm.hip: 256 threads stream
// the two [T] rows, wave 0 reduces the [C] row in the lane / xor-tree order of beam_lm.hip and
// walks the edges.  16 bytes of LDS; every output has one owner, nothing is atomic.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

using namespace asr;

constexpr int FNT = 256;
constexpr int C_MAX = 2048;       // the beam step kernels' widest row
constexpr int T_MAX = 8160;       // asr_tcn_attention_step_f32's longest encoder sequence

struct ForcedParams {
    const float *logits, *att, *cov_in;
    float *cov_out;
    const int32_t *parent, *edge_ptr, *edge_label, *edge_dst, *lens;
    const double *ac_in;
    double *ac_out, *sent_ac;
    int32_t *sent_cov;
    int width, C, T, cov_rows, n_edges, n_out, n_sent;
    float tau;
};

__global__ __launch_bounds__(FNT) void forced_level_kernel(ForcedParams p) {
    __shared__ int cnt_w[FNT / 64];
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, C = p.C;
    int len = p.lens[slot / p.width];
    len = len < 0 ? 0 : (len > T ? T : len);
    int src = p.parent[slot];
    if (src < 0 || src >= p.cov_rows) src = 0;
    int e0 = p.edge_ptr[slot], e1 = p.edge_ptr[slot + 1];
    if (e0 < 0 || e1 > p.n_edges) e1 = e0;                     // a malformed range reads nothing

    // ---- coverage of this prefix: the extended unit's row + this step's alignment ------------
    const float *cin = p.cov_in + (size_t)src * T;
    const float *a = p.att + (size_t)slot * T;
    float *cout = p.cov_out + (size_t)slot * T;
    int cnt = 0;
    for (int t = tid; t < T; t += FNT) {
        const float v = cin[t] + a[t];
        cout[t] = v;
        cnt += (t < len && v > p.tau) ? 1 : 0;
    }
    if (e1 <= e0) return;                                      // dead slot (whole workgroup)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) cnt_w[wave] = cnt;
    __syncthreads();
    if (wave != 0) return;
    const int covered = cnt_w[0] + cnt_w[1] + cnt_w[2] + cnt_w[3];

    // ---- log-partition of the slot's logits, kept as (m, log s) --------------------------------
    const float *row = p.logits + (size_t)slot * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(row[c] - m);
    s = wave_sum(s);
    const float ls = logf(s);

    // ---- the edges: (x - m) - log s, so the class at the maximum loses nothing to |m| ----------
    const double base = p.ac_in[slot];
    for (int e = e0 + lane; e < e1; e += 64) {
        const int lab = p.edge_label[e], dst = p.edge_dst[e];
        if (lab < 0 || lab >= C) continue;
        const double v = base + (double)((row[lab] - m) - ls);
        if (dst >= 0) {
            if (dst < p.n_out) p.ac_out[dst] = v;
        } else {
            const int sent = -1 - dst;
            if (sent >= 0 && sent < p.n_sent) {
                p.sent_ac[sent] = v;
                p.sent_cov[sent] = covered;
            }
        }
    }
}

}  // namespace

extern "C" int asr_forced_level_f32(const float *logits, const float *att, const float *cov_in,
                                    float *cov_out, const int32_t *parent, const int32_t *edge_ptr,
                                    const int32_t *edge_label, const int32_t *edge_dst,
                                    const double *acoustic_in, double *acoustic_out,
                                    const int32_t *enc_lens, int B, int width, int C, int T,
                                    int cov_in_rows, int n_edges, int n_out, int n_sent,
                                    float coverage_tau, double *sent_acoustic, int32_t *sent_covered,
                                    void *stream) {
    if (B <= 0 || width <= 0 || C <= 0 || T <= 0 || cov_in_rows <= 0 || n_edges < 0 || n_out < 0 ||
        n_sent < 0 || (long)B * width > 0x7fffffffL)
        return ASR_EINVAL;
    if (C < 2 || C > C_MAX || T > T_MAX) return ASR_EUNSUPPORTED;
    if (!logits || !att || !cov_in || !cov_out || !parent || !edge_ptr || !edge_label || !edge_dst ||
        !acoustic_in || !acoustic_out || !enc_lens || !sent_acoustic || !sent_covered)
        return ASR_EINVAL;
    if (cov_in == cov_out || att == cov_out || acoustic_in == acoustic_out ||
        sent_acoustic == acoustic_out || sent_acoustic == acoustic_in)
        return ASR_EINVAL;
    ForcedParams p;
    p.logits = logits; p.att = att; p.cov_in = cov_in; p.cov_out = cov_out;
    p.parent = parent; p.edge_ptr = edge_ptr; p.edge_label = edge_label; p.edge_dst = edge_dst;
    p.lens = enc_lens; p.ac_in = acoustic_in; p.ac_out = acoustic_out; p.sent_ac = sent_acoustic;
    p.sent_cov = sent_covered;
    p.width = width; p.C = C; p.T = T; p.cov_rows = cov_in_rows; p.n_edges = n_edges;
    p.n_out = n_out; p.n_sent = n_sent; p.tau = coverage_tau;
    hipLaunchKernelGGL(forced_level_kernel, dim3(B * width), dim3(FNT), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
