// Training scan of the TCN decoder's local attention (reference att_speech/modules/tcn.py:
// 190-230 LocalAttention.scores / forward, driven by AttentionDecoderTCN.forward :357-440):
//
//  asr_tcn_attention_scan_fwd_f32 — the whole recurrence over the label positions
//      l = 0..L-1 in ONE launch: a_l = softmax_t(temperature * (w . tanh(eproj_t + glob_l +
//      (a_{l-1} * filt_l)(t)) + b) + pad_t).  Every alignment is written ([L, B, T]); nothing
//      else is saved.
//  asr_tcn_attention_scan_bwd_f32 — the reverse scan: recomputes h from the saved alignments
//      and carries d a_{l-1} through the location filter.
//
// One workgroup per utterance, resident for the whole scan; the previous alignment, the
// step's filter, w and the per-tile partials live in LDS.  Every reduction has a fixed owner
// and a fixed order (no atomics), so both kernels are bitwise reproducible.  fp32 throughout.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

using namespace asr;

constexpr int NT = 512;               // threads per workgroup (8 waves)
constexpr int KF = 32;                // taps of the location filter
constexpr int FS = KF + 1;            // LDS row stride of filt / u (bank-conflict padding)
constexpr int TMAX = 4096;            // longest encoder sequence (LDS plan below)
constexpr int AMAX = 256;             // attention width
constexpr int PART_CAP = 4096;        // forward: partial-score floats for the a-split
constexpr int TILE_CAP = 4096;        // backward: floats of one [TT, A] dh tile
constexpr int TT_MAX = 64;            // backward: frames per tile
constexpr int QMAX = AMAX * KF / NT;  // backward: d_filt accumulators per thread
constexpr float MASKED = -1e5f;

__device__ __forceinline__ float tanh_fast(float x) {
    // tanh(x) = 1 - 2 / (exp(2x) + 1), saturating cleanly at +-1 (as tcn_step.hip)
    const float ex = __expf(2.f * x);
    return 1.f - 2.f / (ex + 1.f);
}

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }

struct ScanParams {
    const float *eproj, *filt, *glob, *a0, *w_score, *b_score, *att, *d_att;
    const int32_t *lens;
    int T, B, L, A;
    int G, AC;          // forward: a-split into G chunks of AC units
    int TT, G2, AC2;    // backward: frames per tile, a-chunks per tile, units per chunk
    float temperature;
    float *att_out, *d_eproj, *d_filt, *d_glob, *d_a0, *d_wb;
};

// ---------------------------------------------------------------------------------------
// forward: per step, work item (t, ag) = 32-tap window of frame t times AC filter rows;
// the G partial scores of a frame are summed in chunk order by the frame's owner.
__global__ __launch_bounds__(NT) void scan_fwd_kernel(ScanParams p) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = p.T, B = p.B, A = p.A, G = p.G, AC = p.AC;
    const int TP = (KF - 1 + T + 3) & ~3;
    float *aprev = smem;                                  // [KF-1 zeros][T]
    float *part = aprev + TP;                             // [max(G * T, T)]
    float *filt = part + ((max(G * T, T) + 3) & ~3);      // [A][FS]
    float *glob = filt + A * FS;                          // [A]
    float *w = glob + A;                                  // [A]
    float *red = w + A;                                   // [32]
    const int len = p.lens[b];
    const float bsc = p.b_score[0];
    for (int i = tid; i < A; i += NT) w[i] = p.w_score[i];
    for (int i = tid; i < KF - 1 + T; i += NT)
        aprev[i] = i < KF - 1 ? 0.f : p.a0[(size_t)(i - (KF - 1)) * B + b];

    for (int l = 0; l < p.L; ++l) {
        const float *fl = p.filt + ((size_t)l * B + b) * A * KF;
        for (int i = tid; i < A * KF; i += NT) filt[(i / KF) * FS + (i % KF)] = fl[i];
        const float *gl = p.glob + ((size_t)l * B + b) * A;
        for (int i = tid; i < A; i += NT) glob[i] = gl[i];
        __syncthreads();
        for (int it = tid; it < G * T; it += NT) {
            const int t = it % T, ag = it / T;
            float win[KF];
#pragma unroll
            for (int j = 0; j < KF; ++j) win[j] = aprev[t + j];      // a_{l-1}[t - (KF-1) + j]
            const float *ep = p.eproj + ((size_t)t * B + b) * A;
            const int a1 = min(A, (ag + 1) * AC);
            float e = 0.f;
            for (int a = ag * AC; a < a1; ++a) {
                const float *f = filt + a * FS;
                float h = ep[a] + glob[a];
#pragma unroll
                for (int j = 0; j < KF; ++j) h = fmaf(win[j], f[j], h);
                e = fmaf(w[a], tanh_fast(h), e);
            }
            part[ag * T + t] = e;
        }
        __syncthreads();
        float emax = -INFINITY;
        for (int t = tid; t < T; t += NT) {
            float e = part[t];
            for (int ag = 1; ag < G; ++ag) e += part[ag * T + t];
            e = (e + bsc) * p.temperature + (t >= len ? MASKED : 0.f);
            part[t] = e;
            emax = fmaxf(emax, e);
        }
        emax = block_max(emax, red);
        float sum = 0.f;
        for (int t = tid; t < T; t += NT) {
            const float v = __expf(part[t] - emax);
            part[t] = v;
            sum += v;
        }
        sum = block_sum(sum, red);
        const float inv = 1.f / sum;
        float *out = p.att_out + ((size_t)l * B + b) * T;
        for (int t = tid; t < T; t += NT) {
            const float v = part[t] * inv;
            out[t] = v;
            aprev[KF - 1 + t] = v;                        // the next step's previous alignment
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------
// backward, in reverse over l.  Per step: g = dA_l + carry, ds = temperature * a (g - <a, g>);
// then per tile of TT frames
//   A: items (tl, ag) recompute h for AC2 units, dh = ds w (1 - tanh^2) and ds tanh into
//      LDS tiles, d_eproj[t, a] += dh (fixed owner, in l order);
//   B: d_glob / d w owners (thread a) sum the tile over t; d_filt owners (a, j) add
//      sum_t dh[t, a] a_{l-1}[t - 31 + j]; u[t, j] = sum_a dh[t, a] filt[a, j];
//   C: carry_{l-1}[t - 31 + j] += u[t, j], summed over j by the owner of the frame.
__global__ __launch_bounds__(NT) void scan_bwd_kernel(ScanParams p) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = p.T, B = p.B, A = p.A, TT = p.TT, G2 = p.G2, AC2 = p.AC2;
    const int AP = A + 1;
    const int TP = (KF - 1 + T + TT + 3) & ~3;
    const int T4 = (T + 3) & ~3;
    float *aprev = smem;                  // [KF-1 zeros][T][TT zeros]
    float *X = aprev + TP;                // [T] a_l
    float *Y = X + T4;                    // [T] g, then ds
    float *carry = Y + T4;                // [T]
    float *filt = carry + T4;             // [A][FS]
    float *w = filt + A * FS;             // [A]
    float *glob = w + A;                  // [A]
    float *dhT = glob + A;                // [TT][AP]
    float *thT = dhT + TT * AP;           // [TT][AP] ds * tanh
    float *uT = thT + TT * AP;            // [TT][FS]
    float *red = uT + TT * FS;            // [32]
    for (int i = tid; i < A; i += NT) w[i] = p.w_score[i];
    for (int i = tid; i < TP; i += NT) aprev[i] = 0.f;
    for (int i = tid; i < T; i += NT) carry[i] = 0.f;
    float wacc = 0.f, bacc = 0.f;         // d w[tid] over all steps; this thread's share of d b
    const int nq = A * KF;

    for (int l = p.L - 1; l >= 0; --l) {
        const size_t row = (size_t)l * B + b;
        const float *fl = p.filt + row * A * KF;
        __syncthreads();                  // previous step's readers of filt / aprev / carry done
        for (int i = tid; i < nq; i += NT) filt[(i / KF) * FS + (i % KF)] = fl[i];
        for (int i = tid; i < A; i += NT) glob[i] = p.glob[row * A + i];
        const float *al = p.att + row * T;
        const float *dl = p.d_att + row * T;
        float dot = 0.f;
        for (int t = tid; t < T; t += NT) {
            const float a = al[t], g = dl[t] + carry[t];
            X[t] = a;
            Y[t] = g;
            carry[t] = 0.f;
            dot = fmaf(a, g, dot);
            aprev[KF - 1 + t] = l > 0 ? p.att[(row - B) * T + t] : p.a0[(size_t)t * B + b];
        }
        dot = block_sum(dot, red);        // (synchronises)
        for (int t = tid; t < T; t += NT) {
            const float ds = p.temperature * (X[t] * (Y[t] - dot));
            Y[t] = ds;
            bacc += ds;
        }
        float qacc[QMAX];
#pragma unroll
        for (int k = 0; k < QMAX; ++k) qacc[k] = 0.f;
        float gacc = 0.f;
        __syncthreads();

        for (int t0 = 0; t0 < T; t0 += TT) {
            // ---- A: recompute h, dh, ds * tanh for the tile
            if (tid < TT * G2) {
                const int tl = tid % TT, ag = tid / TT;
                const int t = t0 + tl;
                const int a0 = ag * AC2, a1 = min(A, a0 + AC2);
                if (t < T) {
                    float win[KF];
#pragma unroll
                    for (int j = 0; j < KF; ++j) win[j] = aprev[t + j];
                    const float ds = Y[t];
                    const size_t eo = ((size_t)t * B + b) * A;
                    const float *ep = p.eproj + eo;
                    float *dep = p.d_eproj + eo;
                    for (int a = a0; a < a1; ++a) {
                        const float *f = filt + a * FS;
                        float h = ep[a] + glob[a];
#pragma unroll
                        for (int j = 0; j < KF; ++j) h = fmaf(win[j], f[j], h);
                        const float th = tanh_fast(h);
                        const float dh = ds * w[a] * (1.f - th * th);
                        dhT[tl * AP + a] = dh;
                        thT[tl * AP + a] = ds * th;
                        dep[a] = l == p.L - 1 ? dh : dep[a] + dh;
                    }
                } else {
                    for (int a = a0; a < a1; ++a) {
                        dhT[tl * AP + a] = 0.f;
                        thT[tl * AP + a] = 0.f;
                    }
                }
            }
            __syncthreads();
            // ---- B: tile reductions over t
            if (tid < A) {
                float sg = 0.f, sw = 0.f;
                for (int tl = 0; tl < TT; ++tl) {
                    sg += dhT[tl * AP + tid];
                    sw += thT[tl * AP + tid];
                }
                gacc += sg;
                wacc += sw;
            }
#pragma unroll
            for (int k = 0; k < QMAX; ++k) {
                const int q = tid + k * NT;
                if (q < nq) {
                    const int a = q / KF, j = q % KF;
                    const float *ap = aprev + t0 + j;
                    float s = 0.f;
                    for (int tl = 0; tl < TT; ++tl) s = fmaf(dhT[tl * AP + a], ap[tl], s);
                    qacc[k] += s;
                }
            }
            for (int it = tid; it < TT * KF; it += NT) {
                const int tl = it / KF, j = it % KF;
                const float *d = dhT + tl * AP;
                float s = 0.f;
                for (int a = 0; a < A; ++a) s = fmaf(d[a], filt[a * FS + j], s);
                uT[tl * FS + j] = s;
            }
            __syncthreads();
            // ---- C: carry into a_{l-1}: frame s = t0 + r - (KF-1) collects u[r - j][j]
            if (tid < TT + KF - 1) {
                const int r = tid, s = t0 + r - (KF - 1);
                if (s >= 0 && s < T) {
                    float c = 0.f;
                    const int jlo = max(0, r - TT + 1), jhi = min(KF - 1, r);
                    for (int j = jlo; j <= jhi; ++j) c += uT[(r - j) * FS + j];
                    carry[s] += c;
                }
            }
            // the next tile's phase-A barrier orders C before the next B rewrites uT
        }
        // ---- the step's filter / global gradients
        float *df = p.d_filt + row * nq;
#pragma unroll
        for (int k = 0; k < QMAX; ++k) {
            const int q = tid + k * NT;
            if (q < nq) df[q] = qacc[k];
        }
        if (tid < A) p.d_glob[row * A + tid] = gacc;
    }
    __syncthreads();
    for (int t = tid; t < T; t += NT) p.d_a0[(size_t)t * B + b] = carry[t];
    if (tid < A) p.d_wb[(size_t)b * (A + 1) + tid] = wacc;
    bacc = block_sum(bacc, red);
    if (tid == 0) p.d_wb[(size_t)b * (A + 1) + A] = bacc;
}

// forward a-split: G chunks minimising passes x chunk cost, with G * T <= PART_CAP (or G = 1)
void fwd_split(int T, int A, int *G, int *AC) {
    int bg = 1;
    long best = -1;
    for (int g = 1; g <= A; ++g) {
        if (g > 1 && (long)g * T > PART_CAP) break;
        const int ac = cdiv(A, g);
        if (g > 1 && cdiv(A, g - 1) == ac) continue;
        const long cost = (long)cdiv(g * T, NT) * (ac * (KF + 8) + 2 * KF);
        if (best < 0 || cost < best) { best = cost; bg = g; }
    }
    *G = bg;
    *AC = cdiv(A, bg);
}

size_t fwd_lds(int T, int A, int G) {
    const size_t TP = (KF - 1 + T + 3) & ~3;
    const size_t part = ((size_t)(G * T > T ? G * T : T) + 3) & ~3;
    return (TP + part + (size_t)A * FS + 2 * A + 32) * sizeof(float);
}

void bwd_tiles(int A, int *TT, int *G2, int *AC2) {
    int tt = TILE_CAP / A;
    tt = tt > TT_MAX ? TT_MAX : (tt < 1 ? 1 : tt);
    int g2 = NT / tt;
    g2 = g2 > A ? A : (g2 < 1 ? 1 : g2);
    *TT = tt;
    *AC2 = cdiv(A, g2);
    *G2 = cdiv(A, *AC2);
}

size_t bwd_lds(int T, int A, int TT) {
    const size_t TP = (KF - 1 + T + TT + 3) & ~3;
    const size_t T4 = (T + 3) & ~3;
    return (TP + 3 * T4 + (size_t)A * FS + 2 * A + 2 * (size_t)TT * (A + 1) + (size_t)TT * FS + 32) *
           sizeof(float);
}

int check_shapes(int T, int B, int L, int A, int Kf) {
    if (T <= 0 || B <= 0 || L <= 0 || A <= 0) return ASR_EINVAL;
    if (Kf != KF || A > AMAX || T > TMAX) return ASR_EUNSUPPORTED;
    return ASR_OK;
}

int launch(void (*kern)(ScanParams), const ScanParams &p, int B, size_t lds, void *stream) {
    if (lds > 160 * 1024) return ASR_EUNSUPPORTED;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return ASR_EUNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3(B), dim3(NT), lds, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

}  // namespace

extern "C" int asr_tcn_attention_scan_fwd_f32(const float *eproj, const float *filt,
                                              const float *glob, const float *a0,
                                              const float *w_score, const float *b_score,
                                              float temperature, const int32_t *enc_lens,
                                              int T, int B, int L, int A, int Kf, float *att,
                                              void *stream) {
    const int rc = check_shapes(T, B, L, A, Kf);
    if (rc != ASR_OK) return rc;
    if (!eproj || !filt || !glob || !a0 || !w_score || !b_score || !enc_lens || !att)
        return ASR_EINVAL;
    ScanParams p = {};
    p.eproj = eproj; p.filt = filt; p.glob = glob; p.a0 = a0; p.w_score = w_score;
    p.b_score = b_score; p.lens = enc_lens;
    p.T = T; p.B = B; p.L = L; p.A = A; p.temperature = temperature;
    fwd_split(T, A, &p.G, &p.AC);
    p.att_out = att;
    return launch(scan_fwd_kernel, p, B, fwd_lds(T, A, p.G), stream);
}

extern "C" int asr_tcn_attention_scan_bwd_f32(const float *eproj, const float *filt,
                                              const float *glob, const float *a0,
                                              const float *w_score, float temperature,
                                              const int32_t *enc_lens, const float *att,
                                              const float *d_att, int T, int B, int L, int A,
                                              int Kf, float *d_eproj, float *d_filt,
                                              float *d_glob, float *d_a0, float *d_wb,
                                              void *stream) {
    const int rc = check_shapes(T, B, L, A, Kf);
    if (rc != ASR_OK) return rc;
    if (!eproj || !filt || !glob || !a0 || !w_score || !enc_lens || !att || !d_att || !d_eproj ||
        !d_filt || !d_glob || !d_a0 || !d_wb)
        return ASR_EINVAL;
    ScanParams p = {};
    p.eproj = eproj; p.filt = filt; p.glob = glob; p.a0 = a0; p.w_score = w_score;
    p.att = att; p.d_att = d_att; p.lens = enc_lens;
    p.T = T; p.B = B; p.L = L; p.A = A; p.temperature = temperature;
    bwd_tiles(A, &p.TT, &p.G2, &p.AC2);
    p.d_eproj = d_eproj; p.d_filt = d_filt; p.d_glob = d_glob; p.d_a0 = d_a0; p.d_wb = d_wb;
    return launch(scan_bwd_kernel, p, B, bwd_lds(T, A, p.TT), stream);
}
