// Label scan of the RNN attention decoder (reference att_speech/modules/decoders/
// attention_decoder.py: Attention.forward :90-111 inside AttentionDecoderRNN.forward :217-232
// and .decode :324-337): additive attention -> context -> one GRU cell, position after position.
//
//  asr_att_gru_scan_fwd_f32 — all L label positions of one hypothesis in ONE launch:
//      rec_l = W_rec h_{l-1};  a_l = softmax_t(v . tanh(eproj_t + rec_l) + b + pad_t);
//      c_l = sum_t a_l[t] encoded_t;  h_l = GRU([emb_l ; c_l], h_{l-1}) with the embedding half
//      of the input projection handed in as gx_emb (teacher forcing: one product outside).
//  asr_att_gru_scan_bwd_f32 — the reverse scan.  tanh is recomputed from the saved rec_l; the
//      GRU cell is differentiated from its saved gate record (r, z, n, hn).
//
// One workgroup per hypothesis, resident for the whole scan; hypotheses are independent, so
// nothing waits or spins.  Matrix-vector products stream their fp32 weights from L2 one wave
// per block of rows (lanes along the columns, 16-byte loads); eproj and encoded are streamed
// one wave per frame.  Every reduction has a fixed owner and a fixed order (no atomics): both
// kernels are bitwise reproducible.  fp32 throughout.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

using namespace asr;

constexpr int NT = 1024;              // threads per workgroup
constexpr int NW = NT / 64;           // waves
constexpr int TMAX = 4096;            // longest encoder sequence
constexpr int HMAX = 320;             // GRU width
constexpr int AMAX = 320;             // attention width
constexpr int EMAX = 512;             // encoder width
constexpr int ASLOT = AMAX / 64;      // attention units per lane
constexpr int ESLOT = EMAX / 64;      // encoder features per lane
constexpr int CG = 8;                 // frame groups of the context sum
constexpr int R = 4;                  // rows per wave and pass of a matrix-vector product

__device__ __forceinline__ float tanh_fast(float x) {
    // tanh(x) = 1 - 2 / (exp(2x) + 1), saturating cleanly at +-1 (as tcn_train.hip)
    const float ex = __expf(2.f * x);
    return 1.f - __fdividef(2.f, ex + 1.f);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// out[r] = sum_k W[r, k] x[k] for r < nrows; W row-major [nrows, ncols] in global memory
// (ncols % 4 == 0), x and out in LDS.  Wave w owns rows w*R .. w*R+R-1, + NW*R, ...
__device__ __forceinline__ void matvec(const float *__restrict__ W, int nrows, int ncols,
                                       const float *x, float *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc4 = ncols >> 2;
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    for (int r0 = wave * R; r0 < nrows; r0 += NW * R) {
        float acc[R];
        const float4 *w4[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            acc[i] = 0.f;
            const int r = min(r0 + i, nrows - 1);         // (clamped rows are not written)
            w4[i] = reinterpret_cast<const float4 *>(W + (size_t)r * ncols);
        }
        for (int k = lane; k < nc4; k += 64) {
            const float4 xv = x4[k];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const float4 w = w4[i][k];
                acc[i] = fmaf(w.x, xv.x, fmaf(w.y, xv.y, fmaf(w.z, xv.z, fmaf(w.w, xv.w, acc[i]))));
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float s = wave_sum(acc[i]);
            if (lane == 0 && r0 + i < nrows) out[r0 + i] = s;
        }
    }
}

struct ScanParams {
    // operands
    const float *eproj, *encoded, *gx_emb, *w_ic, *w_hh, *b_hh, *w_rec, *w_score, *b_score, *h0;
    const int32_t *lens;
    int T, B, beam, L, A, E, H;
    // forward outputs (ctxs, gates, rec may be null: decode keeps nothing)
    float *att, *states, *ctxs, *gates, *rec;
    // backward operands: transposed weights, saved tensors, incoming gradients (may be null)
    const float *w_icT, *w_hhT, *w_recT, *s_att, *s_states, *s_gates, *s_rec, *d_att, *d_states;
    // backward outputs
    float *d_eproj, *d_gates, *d_ctx, *d_rec, *d_v, *d_h0;
};

__device__ __forceinline__ int clamp_len(int len, int T) { return len <= 0 || len > T ? T : len; }

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void scan_fwd_kernel(ScanParams p) {
    __shared__ __attribute__((aligned(16))) float h[HMAX];
    __shared__ __attribute__((aligned(16))) float rec[AMAX];
    __shared__ __attribute__((aligned(16))) float ctx[EMAX];
    __shared__ __attribute__((aligned(16))) float part[CG * EMAX];
    __shared__ float sc[TMAX];
    __shared__ float gi[3 * HMAX];
    __shared__ float gh[3 * HMAX];
    __shared__ float red[32];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, B = p.B, A = p.A, E = p.E, H = p.H;
    const int NU = B / p.beam, u = b / p.beam;
    const int len = clamp_len(p.lens[u], T);
    const float bsc = p.b_score[0];
    float v[ASLOT];
#pragma unroll
    for (int j = 0; j < ASLOT; ++j) v[j] = lane + 64 * j < A ? p.w_score[lane + 64 * j] : 0.f;
    for (int i = tid; i < H; i += NT) h[i] = p.h0[(size_t)b * H + i];
    __syncthreads();

    for (int l = 0; l < p.L; ++l) {
        const size_t row = (size_t)l * B + b;
        // ---- rec = W_rec h_{l-1}
        matvec(p.w_rec, A, H, h, rec);
        __syncthreads();
        if (p.rec)
            for (int i = tid; i < A; i += NT) p.rec[row * A + i] = rec[i];
        // ---- scores: one wave per frame, lanes along the attention units
        float rc[ASLOT];
#pragma unroll
        for (int j = 0; j < ASLOT; ++j) rc[j] = lane + 64 * j < A ? rec[lane + 64 * j] : 0.f;
        for (int t = wave; t < len; t += NW) {
            const float *ep = p.eproj + ((size_t)t * NU + u) * A;
            float e = 0.f;
#pragma unroll
            for (int j = 0; j < ASLOT; ++j) {
                const int a = lane + 64 * j;
                if (a < A) e = fmaf(v[j], tanh_fast(ep[a] + rc[j]), e);
            }
            e = wave_sum(e);
            if (lane == 0) sc[t] = e + bsc;
        }
        __syncthreads();
        // ---- softmax over the utterance's own frames (padding scores -1e5 lower: exactly 0)
        float emax = -INFINITY;
        for (int t = tid; t < len; t += NT) emax = fmaxf(emax, sc[t]);
        emax = block_max(emax, red);
        float sum = 0.f;
        for (int t = tid; t < len; t += NT) {
            const float x = __expf(sc[t] - emax);
            sc[t] = x;
            sum += x;
        }
        sum = block_sum(sum, red);
        const float inv = 1.f / sum;
        float *out = p.att + row * T;
        for (int t = tid; t < T; t += NT) {
            const float x = t < len ? sc[t] * inv : 0.f;
            if (t < len) sc[t] = x;
            out[t] = x;
        }
        __syncthreads();
        // ---- context: CG frame groups x E/4 feature quads, then the groups in order
        const int E4 = E >> 2;
        if (tid < CG * E4) {
            const int g = tid / E4, q = tid % E4;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = g; t < len; t += CG) {
                const float a = sc[t];
                const float4 x =
                    reinterpret_cast<const float4 *>(p.encoded + ((size_t)t * NU + u) * E)[q];
                acc.x = fmaf(a, x.x, acc.x);
                acc.y = fmaf(a, x.y, acc.y);
                acc.z = fmaf(a, x.z, acc.z);
                acc.w = fmaf(a, x.w, acc.w);
            }
            reinterpret_cast<float4 *>(part + g * E)[q] = acc;
        }
        __syncthreads();
        for (int e = tid; e < E; e += NT) {
            float s = part[e];
#pragma unroll
            for (int g = 1; g < CG; ++g) s += part[g * E + e];
            ctx[e] = s;
            if (p.ctxs) p.ctxs[row * E + e] = s;
        }
        __syncthreads();
        // ---- GRU cell (torch.nn.GRU: r, z add both halves before the sigmoid; r multiplies
        //      W_hn h + b_hn alone)
        matvec(p.w_ic, 3 * H, E, ctx, gi);
        matvec(p.w_hh, 3 * H, H, h, gh);
        __syncthreads();
        for (int j = tid; j < H; j += NT) {
            const float *gx = p.gx_emb + row * 3 * H;
            const float r = sigmoidf(gx[j] + gi[j] + gh[j] + p.b_hh[j]);
            const float z = sigmoidf(gx[H + j] + gi[H + j] + gh[H + j] + p.b_hh[H + j]);
            const float hn = gh[2 * H + j] + p.b_hh[2 * H + j];
            const float n = tanhf(gx[2 * H + j] + gi[2 * H + j] + r * hn);
            const float hv = (1.f - z) * n + z * h[j];
            if (p.gates) {
                float *g = p.gates + row * 4 * H;
                g[j] = r;
                g[H + j] = z;
                g[2 * H + j] = n;
                g[3 * H + j] = hn;
            }
            p.states[row * H + j] = hv;
            h[j] = hv;                  // only thread j reads h[j] in this phase
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------
// backward, in reverse over l; carry = d h_{l-1} collected from the GRU cell (z path, W_hh^T)
// and from the attention of position l (W_rec^T).
__global__ __launch_bounds__(NT) void scan_bwd_kernel(ScanParams p) {
    __shared__ __attribute__((aligned(16))) float dgi[3 * HMAX];   // (dr, dz, dn) pre-activation
    __shared__ __attribute__((aligned(16))) float dgh[3 * HMAX];   // (dr, dz, dn r)
    __shared__ __attribute__((aligned(16))) float dc[EMAX];
    __shared__ __attribute__((aligned(16))) float drec[AMAX];
    __shared__ float tmp[HMAX];
    __shared__ float carry[HMAX];
    __shared__ float ds[TMAX];
    __shared__ float part[NW * AMAX];
    __shared__ float red[32];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, B = p.B, A = p.A, E = p.E, H = p.H;
    const int len = clamp_len(p.lens[b], T);
    float v[ASLOT], dv[ASLOT];
#pragma unroll
    for (int j = 0; j < ASLOT; ++j) {
        v[j] = lane + 64 * j < A ? p.w_score[lane + 64 * j] : 0.f;
        dv[j] = 0.f;
    }
    for (int i = tid; i < H; i += NT) carry[i] = 0.f;
    __syncthreads();

    for (int l = p.L - 1; l >= 0; --l) {
        const size_t row = (size_t)l * B + b;
        // ---- GRU cell
        for (int j = tid; j < H; j += NT) {
            const float *g = p.s_gates + row * 4 * H;
            const float r = g[j], z = g[H + j], n = g[2 * H + j], hn = g[3 * H + j];
            const float hp = l > 0 ? p.s_states[(row - B) * H + j] : p.h0[(size_t)b * H + j];
            const float dh = carry[j] + (p.d_states ? p.d_states[row * H + j] : 0.f);
            const float dn = dh * (1.f - z) * (1.f - n * n);
            const float dz = dh * (hp - n) * z * (1.f - z);
            const float dr = dn * hn * r * (1.f - r);
            dgi[j] = dr; dgi[H + j] = dz; dgi[2 * H + j] = dn;
            dgh[j] = dr; dgh[H + j] = dz; dgh[2 * H + j] = dn * r;
            float *o = p.d_gates + row * 4 * H;
            o[j] = dr; o[H + j] = dz; o[2 * H + j] = dn; o[3 * H + j] = dn * r;
            carry[j] = dh * z;          // only thread j touches carry[j] here
        }
        __syncthreads();
        matvec(p.w_icT, E, 3 * H, dgi, dc);
        matvec(p.w_hhT, H, 3 * H, dgh, tmp);
        __syncthreads();
        for (int i = tid; i < E; i += NT) p.d_ctx[row * E + i] = dc[i];
        for (int j = tid; j < H; j += NT) carry[j] += tmp[j];
        // ---- g_t = <encoded_t, d c> + incoming alignment gradient: one wave per frame
        float dcr[ESLOT];
#pragma unroll
        for (int j = 0; j < ESLOT; ++j) dcr[j] = lane + 64 * j < E ? dc[lane + 64 * j] : 0.f;
        for (int t = wave; t < len; t += NW) {
            const float *en = p.encoded + ((size_t)t * B + b) * E;
            float g = 0.f;
#pragma unroll
            for (int j = 0; j < ESLOT; ++j) {
                const int e = lane + 64 * j;
                if (e < E) g = fmaf(en[e], dcr[j], g);
            }
            g = wave_sum(g);
            if (lane == 0) ds[t] = g + (p.d_att ? p.d_att[row * T + t] : 0.f);
        }
        __syncthreads();
        // ---- softmax backward: ds = a (g - <a, g>)
        const float *al = p.s_att + row * T;
        float dot = 0.f;
        for (int t = tid; t < len; t += NT) dot = fmaf(al[t], ds[t], dot);
        dot = block_sum(dot, red);
        for (int t = tid; t < len; t += NT) ds[t] = al[t] * (ds[t] - dot);
        __syncthreads();
        // ---- through tanh: d_eproj (this workgroup owns its utterance's rows), d rec, d v
        float rc[ASLOT], dr_acc[ASLOT];
#pragma unroll
        for (int j = 0; j < ASLOT; ++j) {
            rc[j] = lane + 64 * j < A ? p.s_rec[row * A + lane + 64 * j] : 0.f;
            dr_acc[j] = 0.f;
        }
        for (int t = wave; t < len; t += NW) {
            const size_t eo = ((size_t)t * B + b) * A;
            const float *ep = p.eproj + eo;
            float *dep = p.d_eproj + eo;
            const float d = ds[t];
#pragma unroll
            for (int j = 0; j < ASLOT; ++j) {
                const int a = lane + 64 * j;
                if (a < A) {
                    const float th = tanh_fast(ep[a] + rc[j]);
                    const float dpre = d * v[j] * (1.f - th * th);
                    dep[a] += dpre;             // zero-initialised by the caller; l order
                    dr_acc[j] += dpre;
                    dv[j] = fmaf(d, th, dv[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < ASLOT; ++j)
            if (lane + 64 * j < A) part[wave * A + lane + 64 * j] = dr_acc[j];
        __syncthreads();
        for (int a = tid; a < A; a += NT) {
            float s = part[a];
            for (int w = 1; w < NW; ++w) s += part[w * A + a];
            drec[a] = s;
            p.d_rec[row * A + a] = s;
        }
        __syncthreads();
        matvec(p.w_recT, H, A, drec, tmp);
        __syncthreads();
        for (int j = tid; j < H; j += NT) carry[j] += tmp[j];
        __syncthreads();
    }
    for (int j = tid; j < H; j += NT) p.d_h0[(size_t)b * H + j] = carry[j];
#pragma unroll
    for (int j = 0; j < ASLOT; ++j)
        if (lane + 64 * j < A) part[wave * A + lane + 64 * j] = dv[j];
    __syncthreads();
    for (int a = tid; a < A; a += NT) {
        float s = part[a];
        for (int w = 1; w < NW; ++w) s += part[w * A + a];
        p.d_v[(size_t)b * A + a] = s;
    }
}

int check_shapes(int T, int B, int beam, int L, int A, int E, int H) {
    if (T <= 0 || B <= 0 || beam <= 0 || L <= 0 || A <= 0 || E <= 0 || H <= 0) return ASR_EINVAL;
    if (B % beam != 0) return ASR_EINVAL;
    if (T > TMAX || A > AMAX || E > EMAX || H > HMAX || (A & 3) || (E & 3) || (H & 3))
        return ASR_EUNSUPPORTED;
    return ASR_OK;
}

int launch(void (*kern)(ScanParams), const ScanParams &p, void *stream) {
    hipLaunchKernelGGL(kern, dim3(p.B), dim3(NT), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

}  // namespace

extern "C" int asr_att_gru_scan_fwd_f32(const float *eproj, const float *encoded,
                                        const int32_t *enc_lens, const float *gx_emb,
                                        const float *w_ic, const float *w_hh, const float *b_hh,
                                        const float *w_rec, const float *w_score,
                                        const float *b_score, const float *h0, int T, int B,
                                        int beam, int L, int A, int E, int H, float *att,
                                        float *states, float *contexts, float *gates, float *rec,
                                        void *stream) {
    const int rc = check_shapes(T, B, beam, L, A, E, H);
    if (rc != ASR_OK) return rc;
    if (!eproj || !encoded || !enc_lens || !gx_emb || !w_ic || !w_hh || !b_hh || !w_rec ||
        !w_score || !b_score || !h0 || !att || !states)
        return ASR_EINVAL;
    ScanParams p = {};
    p.eproj = eproj; p.encoded = encoded; p.lens = enc_lens; p.gx_emb = gx_emb; p.w_ic = w_ic;
    p.w_hh = w_hh; p.b_hh = b_hh; p.w_rec = w_rec; p.w_score = w_score; p.b_score = b_score;
    p.h0 = h0;
    p.T = T; p.B = B; p.beam = beam; p.L = L; p.A = A; p.E = E; p.H = H;
    p.att = att; p.states = states; p.ctxs = contexts; p.gates = gates; p.rec = rec;
    return launch(scan_fwd_kernel, p, stream);
}

extern "C" int asr_att_gru_scan_bwd_f32(const float *eproj, const float *encoded,
                                        const int32_t *enc_lens, const float *w_icT,
                                        const float *w_hhT, const float *w_recT,
                                        const float *w_score, const float *h0, const float *att,
                                        const float *states, const float *gates, const float *rec,
                                        const float *d_att, const float *d_states, int T, int B,
                                        int L, int A, int E, int H, float *d_eproj, float *d_gates,
                                        float *d_contexts, float *d_rec, float *d_w_score,
                                        float *d_h0, void *stream) {
    const int rc = check_shapes(T, B, 1, L, A, E, H);
    if (rc != ASR_OK) return rc;
    if (!eproj || !encoded || !enc_lens || !w_icT || !w_hhT || !w_recT || !w_score || !h0 ||
        !att || !states || !gates || !rec || !d_eproj || !d_gates || !d_contexts || !d_rec ||
        !d_w_score || !d_h0)
        return ASR_EINVAL;
    ScanParams p = {};
    p.eproj = eproj; p.encoded = encoded; p.lens = enc_lens; p.w_icT = w_icT; p.w_hhT = w_hhT;
    p.w_recT = w_recT; p.w_score = w_score; p.h0 = h0; p.s_att = att; p.s_states = states;
    p.s_gates = gates; p.s_rec = rec; p.d_att = d_att; p.d_states = d_states;
    p.T = T; p.B = B; p.beam = 1; p.L = L; p.A = A; p.E = E; p.H = H;
    p.d_eproj = d_eproj; p.d_gates = d_gates; p.d_ctx = d_contexts; p.d_rec = d_rec;
    p.d_v = d_w_score; p.d_h0 = d_h0;
    return launch(scan_bwd_kernel, p, stream);
}
