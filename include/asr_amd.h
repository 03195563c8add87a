/*
 * include/asr_amd.h — C ABI of libasr_amd.so (MI355X / gfx950 HIP kernels).
 *
 * The reference (chorowski-lab/pytorch-asr) has no native code and no FFI for
 * this path: its lattice arithmetic is Python-level torch code resolved by name
 * (SURVEY.md §8b).  Each entry point below therefore replaces a *Python*
 * function of the reference; the citation names the file:line (relative to the
 * reference root) whose arithmetic the kernel reproduces.  INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with h_;
 *   - plain pointers and sizes only, no torch / HIP types (the stream is passed
 *     as void* = hipStream_t);
 *   - caller owns every buffer, the library never allocates, never
 *     synchronises, and launches only on the passed stream (graph-capturable);
 *   - return value: ASR_OK or an ASR_E* code; nothing is launched on error;
 *   - tensors are dense row-major; log-probs are TIME-MAJOR [T,B,C] like the
 *     reference (fst_utils.py:329);
 *   - graph matrices are the reference's padded adjacency form
 *     (fst_utils.py:222-294, 491-521) with int32 indices:
 *     [Bg,N,K] with Bg == 1 (shared, e.g. the denominator graph,
 *     fst_utils.py:662-676) or Bg == B; padding arcs carry weight <= neg_inf/2.
 */
#ifndef ASR_AMD_H
#define ASR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    ASR_OK = 0,
    ASR_EINVAL = 1,      /* bad shape / null pointer (reference: AssertionError) */
    ASR_EUNSUPPORTED = 2,/* shape exceeds what the kernels are built for */
    ASR_ELAUNCH = 3      /* HIP reported a launch error */
};

/* Library / ABI version, bumped when a signature changes (23: the noise and non-finite-flag
 * entry points, asr_adam_clip_step_ex_f32). */
int asr_abi_version(void);

/* Human-readable text for an ASR_* code (static storage). */
const char *asr_strerror(int code);

/*
 * Bytes of workspace asr_lattice_fwbw_f32 needs (alphas [T,B,N] f32 plus
 * internal scratch).  Replaces the `lalphas` allocation of
 * PathLogSumExp.forward (fst_utils.py:428).
 */
int64_t asr_lattice_fwbw_workspace_bytes(int T, int B, int C, int N);

/*
 * Log-semiring forward-backward over per-utterance lattices.
 * Replaces PathLogSumExp.forward (fst_utils.py:403-480), reached through
 * path_reduction(..., red_kind in {'logsumexp' with 8 matrices,
 * 'logsumexp_fwb'}) (fst_utils.py:345-347).
 *
 *   lp        [T,B,C] f32   log-probs, time-major
 *   lens      [B]     i32   active frames per utterance, 0 <= lens[b] <= T
 *                           (the reference additionally requires them sorted
 *                           descending, fst_utils.py:432; the kernel does not)
 *   src_in/il_in/w_in   [Bg,N,Kin]  incoming arcs of each state
 *   term                [Bg,N]      terminal log-weights
 *   dst_out/il_out/w_out [Bg,N,Kout] outgoing arcs of each state
 *   out_logZ  [B]     f32   +log-sum of all accepted paths (callers negate)
 *   out_grad  [T,B,C] f32   d logZ[b] / d lp[t,b,c]; rows t >= lens[b] are
 *                           written as zeros (fst_utils.py:448)
 *   out_logZ_bwd [B] f32 or NULL: the backward-pass total used by the
 *                           reference's consistency print (fst_utils.py:475-479)
 *   workspace: asr_lattice_fwbw_workspace_bytes(T,B,C,N) bytes
 */
int asr_lattice_fwbw_f32(const float *lp, int T, int B, int C,
                         const int32_t *lens,
                         const int32_t *src_in, const int32_t *il_in,
                         const float *w_in, const float *term,
                         const int32_t *dst_out, const int32_t *il_out,
                         const float *w_out,
                         int N, int Kin, int Kout, int Bg, float neg_inf,
                         float *out_logZ, float *out_grad,
                         float *out_logZ_bwd,
                         void *workspace, int64_t workspace_bytes,
                         void *stream);

/*
 * The same forward-backward (same arguments, outputs and workspace: replaces
 * PathLogSumExp.forward, fst_utils.py:403-480) for BAND lattices in the rescaled linear
 * domain (ABI v13; csrc/lattice_band.inc): state-labelled graphs whose state n is entered
 * only from {n, n-1, n-2} with arc weights <= 0, N <= 256, C <= 64, Bg == B — the lattices
 * CTCGraphGen builds for mono-character transcripts (fst_utils.py:603-613; the `2 L + 1`
 * CTC chain).  One wave per direction keeps four consecutive states per lane (no
 * transcendental, no LDS and no barrier on the recurrence), alpha / beta are block floating
 * point (one binary exponent per lane, rescaled by exact powers of two), the posterior rows
 * are normalised by Z (every group of four rows is checked to sum to four); only every second
 * alpha / beta row goes through the workspace (the consumer recomputes the one in between).
 *   grad_sign   +1, or -1 for the occupancies of -logZ (see asr_lattice_fwbw_signed_f32; ABI v20)
 *   ctc_labels  NULL, or the transcripts [B, ctc_lmax] (+ ctc_label_lens [B]) the graph matrices were
 *               built from by asr_ctc_graph_build with context_order 1 (N >= 2 ctc_lmax + 1): the
 *               kernel then writes the chain down from the labels and reads the matrices only for
 *               utterances the log-domain body has to redo (ABI v21)
 *   redo_count  device word of the caller or NULL: incremented once per utterance that the
 *               log-domain body had to redo; never reset by the library (a running counter:
 *               the caller takes differences).  (ABI v17)
 * asr_lattice_fwbw_band_supported says whether the SHAPES qualify; the graph of every
 * utterance is checked inside the kernel, and an utterance whose graph has another shape,
 * has no feasible alignment, or whose numbers leave the fp32 range runs the generic
 * log-domain body in the same launch (correct, slow): route here only graphs known to be
 * band-shaped (att_speech._native tags the ones its builders make and checks the others on
 * the host).  ASR_EUNSUPPORTED when the shapes do not qualify.
 */
int asr_lattice_fwbw_band_supported(int T, int B, int C, int N, int Kin, int Kout, int Bg);
int asr_lattice_fwbw_band_f32(const float *lp, int T, int B, int C,
                              const int32_t *lens,
                              const int32_t *src_in, const int32_t *il_in,
                              const float *w_in, const float *term,
                              const int32_t *dst_out, const int32_t *il_out,
                              const float *w_out,
                              int N, int Kin, int Kout, int Bg, float neg_inf, float grad_sign,
                              float *out_logZ, float *out_grad,
                              float *out_logZ_bwd,
                              void *workspace, int64_t workspace_bytes,
                              uint32_t *redo_count,
                              const int32_t *ctc_labels, const int32_t *ctc_label_lens, int ctc_lmax,
                              void *stream);

/*
 * Alpha-only scan: path_reduction's autodiff branch evaluated forward
 * (fst_utils.py:349-397) with reduction logsumexp (viterbi == 0) or max
 * (viterbi == 1, fst_utils.py:366-370).
 * For viterbi == 1 and out_best_il != NULL it also returns the input label of
 * the best path's arc at every frame — what FSTDecoder.decode reads from the
 * autograd gradient as `logits.grad.min(-1)[1]` (advanced_decoder.py:546-554);
 * rows t >= lens[b] are 0.  Ties pick the first maximum.
 *   out_score   [B]   f32
 *   out_best_il [T,B] i32 or NULL
 *   workspace: asr_lattice_viterbi_workspace_bytes(T,B,N) bytes when
 *              out_best_il != NULL, else may be NULL.
 */
int64_t asr_lattice_viterbi_workspace_bytes(int T, int B, int N);

int asr_lattice_forward_f32(const float *lp, int T, int B, int C,
                            const int32_t *lens,
                            const int32_t *src_in, const int32_t *il_in,
                            const float *w_in, const float *term,
                            int N, int K, int Bg, float neg_inf, int viterbi,
                            float *out_score, int32_t *out_best_il,
                            void *workspace, int64_t workspace_bytes,
                            void *stream);

/*
 * Row-wise log-softmax over contiguous groups: x viewed as [rows, group],
 * y = x - logsumexp(x, -1).  Replaces get_normalized_acts
 * (modules/ctc_losses.py:29-43): group = C for the plain branch (:41-42),
 * group = num_symbols for normalize_by_dim = context_order-1 (:34-40,
 * the per-context block-wise normalisation over the last symbol axis).
 * Computed as (x - max) - log sum exp(x - max): a common offset of the row costs no accuracy.
 * -inf entries (masked classes) give -inf; a row of nothing but -inf gives NaN (-inf - -inf),
 * as torch.log_softmax does.  group <= 8192, else ASR_EUNSUPPORTED (all row kernels below too).
 */
int asr_log_softmax_fwd_f32(const float *x, int64_t rows, int group,
                            float *y, void *stream);

/* dx = dy - exp(y) * sum(dy, -1)   (autograd of the above) */
int asr_log_softmax_bwd_f32(const float *y, const float *dy, int64_t rows,
                            int group, float *dx, void *stream);

/*
 * FSTDecoder.get_fst_loss's stabilisation (advanced_decoder.py:479-484):
 *   row_max[t,b] = max_c x[t,b,c];  y = x - row_max;
 *   max_sum[b]   = sum_{t < lens[b]} row_max[t,b]
 * x, y [T,B,C]; row_max [T,B] (required, also the reduction scratch);
 * max_sum [B], summed in a fixed order (bitwise reproducible); lens outside [0, T] are
 * clamped.  A row of nothing but -inf has row_max -inf and y NaN.
 */
int asr_sub_rowmax_f32(const float *x, int T, int B, int C,
                       const int32_t *lens, float *y, float *row_max,
                       float *max_sum, void *stream);

/*
 * Index of the first maximum of every row of x [rows, C]: the per-frame
 * arg-max of CTCDecoderAdvanced.decode (advanced_decoder.py:352,
 * `torch.max(logits_t, 2)`).  out_idx [rows] i32.  Equal values: the lowest index, so a row
 * of nothing but -inf gives 0.  A NaN entry ranks as -inf (torch.max would return it): the
 * result is the first maximum of the other entries, and 0 for a row of nothing but NaN.
 */
int asr_argmax_rows_f32(const float *x, int64_t rows, int C, int32_t *out_idx,
                        void *stream);

/*
 * Device-side construction of the CTC training lattices for a batch of label
 * sequences (context orders 1 and 2), directly in the int32 / f32 layout the
 * lattice entry points take ([B, N = 2*Lmax+1, K = 3], padding arcs at
 * nc_weight).  Replaces get_training_matrices_batch (fst_utils.py:607-613:
 * OpenFst compose per utterance + fst_to_matrices :222-294 +
 * batch_training_graph_matrices :491-521) and the per-step host-to-device copy
 * of the 8 padded tensors (advanced_decoder.py:457-459).
 *   labels [B,Lmax] i32 symbols in [1, num_symbols), already reduced modulo
 *   num_symbols for bigram data sets (fst_utils.py:595-600); label_lens [B].
 */
int asr_ctc_graph_build(const int32_t *labels, const int32_t *label_lens, int B, int Lmax,
                        int num_symbols, int context_order, int allow_nonblank_selfloops,
                        int use_contextual_blanks, float nc_weight, int32_t *src_in,
                        int32_t *il_in, float *w_in, float *term, int32_t *dst_out,
                        int32_t *il_out, float *w_out, void *stream);

/*
 * Forward-backward / alpha scan over GROUP-FACTORED graphs: the reference's CTC
 * decoding graphs (build_ctc_mono_decoding_fst fst_utils.py:679-726,
 * build_ctc_bigram_decoding_fst :729-835), i.e. the denominator graph of the
 * globally normalised loss (advanced_decoder.py:473,497-500) and the search
 * graph of FSTDecoder.decode (:542-554).  State s1 feeds group g_of[s1]; state
 * s2 accepts an arc from every s1 with g_of[s1] == h_of[s2], plus an extra
 * self-loop when selfx[s2]; every arc into s2 consumes label[s2] with weight 0;
 * the start state is 0.  Same results as asr_lattice_fwbw_f32 /
 * asr_lattice_forward_f32 on the equivalent padded arc matrices (up to fp32
 * summation order) at ~1/17 of the arithmetic for the 2401-state bigram graph.
 *   g_of, h_of, label, selfx, uniq [N] i32 (uniq: no other state has this label)
 *   mem_g [G,Wg], mem_h [G,Wh] i32: states of every group, ascending, -1 padded
 *   term [N] f32 terminal log-weights
 * Outputs / workspace as for the generic entry points;
 * workspace: asr_lattice_grouped_workspace_bytes(T,B,N,G).  Needs 16*G <= 1024.
 */
int64_t asr_lattice_grouped_workspace_bytes(int T, int B, int N, int G);

int asr_lattice_grouped_fwbw_f32(
    const float *lp, int T, int B, int C, const int32_t *lens, int N, int G, int Wg, int Wh,
    const int32_t *g_of, const int32_t *h_of, const int32_t *label, const int32_t *selfx,
    const int32_t *uniq, const int32_t *mem_g, const int32_t *mem_h, const float *term,
    float neg_inf, float *out_logZ, float *out_grad, float *out_logZ_bwd, void *workspace,
    int64_t workspace_bytes, void *stream);
/* ... with accumulate != 0: out_grad += occupancies (rows past an utterance's end are left as they
 * are) — the denominator of FSTDecoder.get_fst_loss (advanced_decoder.py:497-500) added onto the
 * numerator's (negated) occupancies in the same buffer: d loss / d acts without a separate
 * [T,B,C] addition (ABI v22). */
int asr_lattice_grouped_fwbw_acc_f32(
    const float *lp, int T, int B, int C, const int32_t *lens, int N, int G, int Wg, int Wh,
    const int32_t *g_of, const int32_t *h_of, const int32_t *label, const int32_t *selfx,
    const int32_t *uniq, const int32_t *mem_g, const int32_t *mem_h, const float *term,
    float neg_inf, int accumulate, float *out_logZ, float *out_grad, float *out_logZ_bwd,
    void *workspace, int64_t workspace_bytes, void *stream);

int asr_lattice_grouped_forward_f32(
    const float *lp, int T, int B, int C, const int32_t *lens, int N, int G, int Wg, int Wh,
    const int32_t *g_of, const int32_t *h_of, const int32_t *label, const int32_t *selfx,
    const int32_t *uniq, const int32_t *mem_g, const int32_t *mem_h, const float *term,
    float neg_inf, int viterbi, float *out_score, int32_t *out_best_il, void *workspace,
    int64_t workspace_bytes, void *stream);

/*
 * Bidirectional, bias-free LSTM recurrence on a padded, length-masked batch —
 * the sequential part of BatchRNN (modules/encoders/encoder_utils.py:55-124:
 * nn.LSTM(bidirectional=True, bias=False) applied to a PackedSequence).
 * The caller supplies the input projection of every frame,
 *   gx [T,B,2,4H] f32, or bf16 with gx_bf16 != 0 (what a bf16 GEMM emits; halves its
 *      1.75 GB output at B=512) = x · W_ihᵀ   (direction-major, gate order i,f,g,o),
 * and the recurrent weights as bf16 (MFMA operands; accumulation, gate arithmetic and
 * the cell state are fp32; the gates SAVED for the backward pass are rounded to bf16):
 * whh [2,4H,H] for the forward pass,
 * whhT [2,H,4H] (transposed) for the backward pass.
 * Utterance b is active at frame t iff t < lens[b]; padding frames emit zeros
 * and carry no gradient, which reproduces pack_padded_sequence semantics
 * (the reverse direction starts at each utterance's own last frame).
 *   y      [T,B,2,H]   per-direction hidden outputs (the reference sums the
 *                      two directions, encoder_utils.py:112-117); may be null when the
 *                      caller only needs the bf16 copy below (inner layers of a stack)
 *   y_bf16 [2,T+2,B,H] bf16 copy, direction-major, frame t at index t+1 with a
 *                      zero frame at both ends: h_{t-1} of the forward
 *                      direction is the slice [0][0:T], of the reverse
 *                      direction [1][2:T+2] — contiguous GEMM operands for dW_hh
 *   gates_bf16 [T,2,B,H,4] bf16 post-activation gates (one 8-byte record i,f,g,o per
 *                      hidden unit), csave [T,2,B,H] f32 cell states: saved by the
 *                      forward pass for the backward pass
 *   dy     [T,B,2,H]   gradient w.r.t. y; dy_shared = 1: [T,B,H], one gradient for
 *                      both directions (BatchRNN sums them, encoder_utils.py:112-117);
 *                      dy_shared is 0 or 1 (ASR_EINVAL otherwise)
 *   dgates_bf16 [T,B,2,4H] bf16: gradient w.r.t. the gate pre-activations
 *                      (= w.r.t. gx); the caller forms dx, dW_ih, dW_hh from it
 *                      with dense GEMMs (bf16 operands, fp32 accumulation)
 * workspace: asr_lstm_workspace_bytes(B, H) bytes.  Hidden sizes built:
 * 64, 128, 256, 320, 384, 512, 768 (ASR_EUNSUPPORTED otherwise).
 *   err_flag  optional device word owned by the caller (never cleared by the library).
 *             The persistent recurrence hands tiles between co-resident workgroups with
 *             bounded spins; if a spin bound expires (another stream's kernel kept a team
 *             mate off the device) the kernel stores 1 here and poisons its outputs with
 *             NaN instead of hanging.  A caller that reads a non-zero word must discard
 *             the step (att_speech._native.lstm_check_errors raises).  Debug knob:
 *             ASR_LSTM_SPIN_LIMIT=<n> overrides the bound (0 forces the timeout).
 */
int64_t asr_lstm_workspace_bytes(int B, int H);

int asr_lstm_bidir_fwd_bf16(const void *gx, int gx_bf16, const void *whh_bf16,
                            const int32_t *lens, int T, int B, int H,
                            float *y, void *y_bf16, void *gates_bf16, float *csave,
                            void *workspace, int64_t workspace_bytes,
                            uint32_t *err_flag, void *stream);

/* Weight gradients of one layer from the gate gradients, in one pass over them (replaces the
 * three chunked library products + sums of the reference's autograd for nn.LSTM weights,
 * encoder_utils.py:78,100):
 *   dgates_bf16 [T*B, 2, 4H]  as written by asr_lstm_bidir_bwd_bf16
 *   x_bf16      [T*B, H] layer input (input size == H), or NULL: then dw_ih must be NULL too
 *               and only dw_hh is computed (first layer: the caller multiplies for dw_ih)
 *   y_bf16      [2, T+2, B, H] the forward call's zero-padded bf16 outputs (h_{t-1} operands)
 *   dw_ih [2*4H, H], dw_hh [2][4H][H]  f32 out (overwritten)
 * Built for H = 320 (asr_lstm_wgrad_supported; ASR_EUNSUPPORTED otherwise).  fp32
 * accumulation over all frames in a fixed order: deterministic. */
int asr_lstm_wgrad_supported(int H);
int64_t asr_lstm_wgrad_workspace_bytes(int T, int B, int H, int with_input);
int asr_lstm_wgrad_bf16(const void *dgates_bf16, const void *x_bf16, const void *y_bf16,
                        int T, int B, int H, float *dw_ih, float *dw_hh,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* Input gradient of one layer from the gate gradients: dx [T*B, H] f32 = dgates [T*B, 2*4H] ·
 * w_ih [2*4H, H] (both bf16, w_ih = nn.LSTM weight_ih_l0 / _reverse stacked; input size == H).
 * Replaces the library product behind asr_lstm_bidir_bwd_bf16.  Built for H = 320. */
int asr_lstm_dgrad_supported(int H);
int asr_lstm_dgrad_bf16(const void *dgates_bf16, const void *w_ih_bf16, int T, int B, int H,
                        float *dx, void *stream);

/* The same layer with the input projection fused into the persistent recurrence
 * (replaces the `x·W_ihᵀ` GEMM in front of asr_lstm_bidir_fwd_bf16 when the layer's input
 * size F equals H, i.e. every BatchRNN after the first, encoder_utils.py:97-124 — or, for
 * H = 320, F = 352: the first layer behind the reference's conv front-end):
 *   x_bf16    [T,B,F] bf16 row-major layer input
 *   wih_bf16  [2 dir][4H][F] bf16, rows in gate order i,f,g,o (nn.LSTM weight_ih_l0 /
 *             weight_ih_l0_reverse stacked)
 *   y         must be NULL when F != H (that variant writes y_bf16 only)
 * Pre-activations are accumulated in fp32 over both products (no bf16 rounding of
 * x·W_ihᵀ).  ASR_EUNSUPPORTED when asr_lstm_fused_supported(B, H, F) returns 0 (hidden
 * size not one of 64/128/256/320, another input size, persistent path switched off; 1
 * otherwise): the caller then uses the GEMM + asr_lstm_bidir_fwd_bf16. */
int asr_lstm_fused_supported(int B, int H, int F);
int asr_lstm_bidir_fwd_fused_bf16(const void *x_bf16, const void *wih_bf16,
                                  const void *whh_bf16, const int32_t *lens,
                                  int T, int B, int H, int F, float *y, void *y_bf16,
                                  void *gates_bf16, float *csave, void *workspace,
                                  int64_t workspace_bytes, uint32_t *err_flag, void *stream);

int asr_lstm_bidir_bwd_bf16(const float *dy, int dy_shared, const void *whhT_bf16,
                            const int32_t *lens, int T, int B, int H,
                            const void *gates_bf16, const float *csave,
                            void *dgates_bf16,
                            void *workspace, int64_t workspace_bytes,
                            uint32_t *err_flag, void *stream);

/*
 * Bidirectional GRU recurrence (bias-free; the recurrent part of a BatchRNN with
 * rnn_type=nn.GRU), the arithmetic of torch.nn.GRU(bias=False) with rows in torch's order
 * r | z | n:
 *   r = σ(gx_r + h·W_hrᵀ)   z = σ(gx_z + h·W_hzᵀ)   hn = h·W_hnᵀ
 *   n = tanh(gx_n + r ⊙ hn)  h' = (1 − z) ⊙ n + z ⊙ h
 * Same contract as the LSTM above: padded input with lens[B] (utterance b is active at
 * frame t iff t < lens[b]; padding frames emit zeros and carry no gradient; the reverse
 * direction starts from the zero state at each utterance's own last frame); bf16 MFMA
 * operands (h, W_hh), fp32 accumulation, gates and state; persistent kernels by default,
 * one launch per step with ASR_LSTM_PERSIST=0 (bit-identical); err_flag and
 * ASR_LSTM_SPIN_LIMIT as for the LSTM.
 *   gx [T,B,2,3H] f32, or bf16 with gx_bf16 != 0: x · W_ihᵀ per direction (gate order r,z,n)
 *   whh [2,3H,H] bf16 for the forward pass, whhT [2,H,3H] (transposed) for the backward pass
 *   y      [T,B,2,H] f32 per-direction outputs (required: the backward pass reads h_{t-1}
 *                    from it)
 *   y_bf16 [2,T+2,B,H] bf16 copy laid out as the LSTM's (h_{t-1} operands for dW_hh)
 *   gates_bf16 [T,2,B,H,4] bf16 records (r, z, n, hn) saved for the backward pass
 *   dy     [T,B,2,H], or [T,B,H] with dy_shared != 0 (one gradient for both directions)
 *   dgx_bf16 [T,B,2,3H] bf16 (dr, dz, dn) pre-activation gradients = gradient w.r.t. gx:
 *                    the operand of dx and dW_ih
 *   dhn_bf16 [T,B,2,H] bf16 dn ⊙ r: with dr, dz the operand [dr, dz, dhn] of dW_hh
 * workspace: asr_gru_workspace_bytes(B, H) bytes.  Hidden sizes built: 64, 128, 256, 320
 * (ASR_EUNSUPPORTED otherwise).  asr_gru_supported(B, H): 0 = not built; bit 0 = runs;
 * bit 1 = the persistent kernels take this shape (else one launch per step).
 */
int64_t asr_gru_workspace_bytes(int B, int H);
int asr_gru_supported(int B, int H);

int asr_gru_bidir_fwd_bf16(const void *gx, int gx_bf16, const void *whh_bf16,
                           const int32_t *lens, int T, int B, int H,
                           float *y, void *y_bf16, void *gates_bf16,
                           void *workspace, int64_t workspace_bytes,
                           uint32_t *err_flag, void *stream);

int asr_gru_bidir_bwd_bf16(const float *dy, int dy_shared, const void *whhT_bf16,
                           const int32_t *lens, int T, int B, int H,
                           const void *gates_bf16, const float *y,
                           void *dgx_bf16, void *dhn_bf16,
                           void *workspace, int64_t workspace_bytes,
                           uint32_t *err_flag, void *stream);

/*
 * BatchNorm2d + Hardtanh(lo, hi) fused over the [B, C, H, W] output of a
 * convolution (fp32, or bf16 with x_bf16 — channels-last only; dx then is bf16 too): the `Normalization('batch_norm')` + `nn.Hardtanh(0, 20)` pair of
 * the DeepSpeech2 conv front-end (deep_speech_2.py:60-73).  training != 0: batch
 * statistics (biased variance for the normalisation; running_mean / running_var
 * updated with `momentum` and the unbiased variance like nn.BatchNorm2d, pass
 * null to leave them alone); training == 0: running statistics.  The clamped
 * activation is written as fp32 or bf16 (out_bf16), in NCHW or time-major
 * [H, B, C, W] order (out_time_major: the permute(2,0,1,3) of
 * deep_speech_2.py:142-146).  channels_last != 0: x (and a non-time-major out /
 * dy, and dx) are stored [B, H, W, C] — the layout MIOpen's implicit-GEMM
 * convolutions produce and consume (C % 4 == 0, C <= 1024 and C/4 must divide 256, i.e. C in
 * {4, 8, ..., 1024}; ASR_EUNSUPPORTED otherwise, and for bf16 x that is not channels-last;
 * a refusal launches nothing and leaves every output and the workspace alone).  save_mean /
 * save_invstd [C] feed the backward.
 * Batch statistics are summed about a per-channel pivot (the channel's first element) in fp32 per
 * workgroup and in double across workgroups: the error of the variance is that of a centred
 * evaluation, depth * 2^-23 * (var + maxdev^2) with maxdev the largest |x - mean| of the channel,
 * whatever |mean| / std is (a folded conv_bias shifts the mean only).
 * A NaN in x stays NaN in out like nn.Hardtanh(nn.BatchNorm2d(x)): that element with running
 * statistics, its whole channel (and that channel's save_mean, dx, dgamma) with batch statistics.
 * Limit: with running statistics the backward's dx is NaN at a NaN x, where torch returns 0.  conv_bias [C] (or null): the bias of the convolution that
 * produced x, added on the fly (x is then the bias-free convolution), so the
 * framework needs neither the broadcast add nor the full-tensor reduction for its
 * gradient; the backward returns that gradient in dconv_bias (may be null).
 * chan_sums (or null): [2][C] doubles, (sum x, sum x^2) per channel of the bias-free input,
 * as the convolution kernels below emit them from their epilogues — the statistics pass
 * over x is then skipped (training only).
 * workspace: asr_bn_act_workspace_bytes(C).
 */
int64_t asr_bn_act_workspace_bytes(int C);
int asr_bn_act_fwd_f32(const void *x, int x_bf16, const float *conv_bias, int B, int C, int H, int W,
                       const float *gamma, const float *beta,
                       float *running_mean, float *running_var,
                       int channels_last,
                       int training, float momentum, float eps, float lo, float hi,
                       void *out, int out_bf16, int out_time_major,
                       float *save_mean, float *save_invstd,
                       const double *chan_sums,
                       void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Backward of the above from the SAVED convolution output x: the Hardtanh mask
 * (lo < bn(x) < hi, torch's hardtanh_backward) is recomputed, dy is read in the
 * dtype / layout the forward wrote.  dx [B,C,H,W] fp32, dgamma / dbeta [C].
 */
int asr_bn_act_bwd_f32(const void *x, int x_bf16, const float *conv_bias, int B, int C, int H, int W,
                       const float *gamma, const float *beta,
                       const float *save_mean, const float *save_invstd,
                       int channels_last,
                       int training, float lo, float hi,
                       const void *dy, int dy_bf16, int dy_time_major,
                       void *dx, float *dgamma, float *dbeta, float *dconv_bias,
                       void *workspace, int64_t workspace_bytes, void *stream);

/*
 * The same backward in two halves, for replicas that share their batch statistics (SyncBN-style
 * data parallelism, att_speech.dp.enable_sync_batchnorm; the single-process reference normalises
 * over the whole batch, deep_speech_2.py:21,60-73) (ABI v19).  phase 1: the per-channel sums
 * {sum dy', sum dy' xhat} of THIS replica as 2 C interleaved doubles at the start of the workspace,
 * and dgamma / dbeta / dconv_bias from them (parameter gradients are local: the gradient
 * all-reduce adds the replicas up); phase 2: dx from the sums the caller left there — all-reduced
 * over the replicas — and n_total, the number of elements per channel they stand for.  phase 0 =
 * asr_bn_act_bwd_f32.
 */
int asr_bn_act_bwd_phase_f32(const void *x, int x_bf16, const float *conv_bias, int B, int C, int H, int W,
                             const float *gamma, const float *beta,
                             const float *save_mean, const float *save_invstd,
                             int channels_last,
                             int training, float lo, float hi,
                             const void *dy, int dy_bf16, int dy_time_major,
                             void *dx, float *dgamma, float *dbeta, float *dconv_bias,
                             void *workspace, int64_t workspace_bytes, int phase, double n_total,
                             void *stream);

/*
 * log_softmax over all C classes followed by the per-frame max stabilisation of
 * FSTDecoder.get_fst_loss (advanced_decoder.py:444-452 with normalize_by_dim = 0, then
 * :479-484) in ONE pass over x [T, B, C]: y = log_softmax(x) - max_c log_softmax(x) = x - max_c x,
 * nls [T, B] = max_c log_softmax(x) (= -log sum_c exp(x - max x)), nls_sum [B] = sum over the
 * frames t < lens[b] of nls — the value the reference subtracts as its denominator when
 * denominator_red = 'none'.  bwd: dx = dy - exp(y + nls) * sum_c dy, the gradient of the
 * log-softmax (the reference detaches the maximum), from the shifted y itself.
 * y is the fp32 difference x - max_c x, correctly rounded; -inf entries stay -inf and take no
 * gradient; a row of nothing but -inf gives y = NaN and nls = NaN.  lens as in asr_sub_rowmax_f32.
 */
int asr_log_softmax_shift_fwd_f32(const float *x, int T, int B, int C, const int32_t *lens,
                                  float *y, float *nls, float *nls_sum, void *stream);
int asr_log_softmax_shift_bwd_f32(const float *y, const float *nls, const float *dy, int64_t rows,
                                  int C, float *dx, void *stream);

/* asr_log_softmax_shift_bwd_f32 for the split-bf16 class projection behind it (wide alphabets):
 * the gradient leaves as dx = hi + lo, two bf16 tensors [rows, ld] (ld >= C, ld <= 2560; columns
 * >= C zero) — the fp32 tensor is never written — together with its column sums (the
 * projection's bias gradient) as asr_log_softmax_shift_bwd_split_blocks(rows) partial rows
 * colsum_partial [blocks, ld], which the caller adds up (asr_sum_leading_f32).  (ABI v15) */
int asr_log_softmax_shift_bwd_split_blocks(int64_t rows);
int asr_log_softmax_shift_bwd_split_bf16(const float *y, const float *nls, const float *dy,
                                         int64_t rows, int C, void *hi_bf16, void *lo_bf16, int ld,
                                         float *colsum_partial, void *stream);

/*
 * out[e] = sum over g < G of in[g * n + e] (n % 4 == 0): the sum of the partial products of a
 * weight-gradient GEMM split over chunks of frames (torch's strided reduction reads at
 * 1.4 TB/s here).  Summed over g in that order in fp32 (bitwise reproducible).  in and out
 * must be 16-byte aligned (float4 accesses), else ASR_EINVAL.
 */
int asr_sum_leading_f32(const float *in, int G, int64_t n, float *out, void *stream);

/*
 * x = hi + lo, hi = bf16(x) (round to nearest even), lo = bf16(x - hi): the operands of the
 * split-bf16 class projection of the decoders (advanced_decoder.py:79-223 computes
 * `F.linear(frames, weight, bias)` in fp32; with C = 2401 classes the three bf16 MFMA products
 * hi hi + hi lo + lo hi, accumulated in fp32, stand for it at 2^-16 relative error per term).
 *   x [rows, cols] f32 with row stride ldx (elements); hi / lo [rows, cols] bf16 with row
 *   strides ldhi / ldlo — strided so that the halves can be written straight into the
 *   K-concatenated operand [rows, 3 cols].  A contiguous tensor is one row of n elements.
 * Zeros keep their sign in hi (lo = +0), denormals are split like any value, NaN gives NaN in
 * both halves.  hi + lo is NOT x for +-inf (hi = +-inf, lo = inf - inf = NaN) nor for finite
 * |x| >= 0x7f7f8000 (3.3961775e38), which round to hi = +-inf with lo = -+inf.
 * (ABI v14)
 */
int asr_split_bf16_f32(const float *x, int64_t rows, int64_t cols, int64_t ldx,
                       void *hi_bf16, int64_t ldhi, void *lo_bf16, int64_t ldlo, void *stream);

/*
 * The 7x7, 32 -> 32 channel convolution of the DeepSpeech2 front-end (reference
 * att_speech/modules/encoders/deep_speech_2.py:60-73, Conv2d(32, 32, (7, 7), stride
 * (stride_h, 1)), stride_h in {1, 3}) on channels-last bf16 with fp32 accumulation, bias-free
 * (the bias is folded into asr_bn_act_*):
 *   x [B, H, W, 32] bf16, w [32, 32, 7, 7] f32 (nn.Conv2d layout), y [B, Ho, Wo, 32] bf16,
 *   Ho = (H - 7) / stride_h + 1, Wo = W - 6 (<= 48).
 * fwd: y = conv(x, w);  bwd_data: dx = conv_transpose(dy, w) [B, H, W, 32] bf16;
 * wgrad: dw [32, 32, 7, 7] f32 = sum over the batch of dy (x) x (overwritten).
 * chan_sums (or null): [2][32] doubles, per output channel the sum and the sum of squares of
 * the bf16 outputs — what the following BatchNorm needs (asr_bn_act_fwd_f32).
 * workspace: asr_conv7x7c32_workspace_bytes() (packed weight fragments / partial sums).
 * asr_conv7x7c32_supported(B, H, W, stride_h): 1 if all three entry points take the shape, 0
 * if one of them answers ASR_EINVAL / ASR_EUNSUPPORTED (the launchers run the same checks).
 * That is stride_h = 3, 7 <= W <= 48 without W = 12, 14, 15 and 20 (the LDS row pitch picked
 * against bank conflicts overruns the forward kernel's LDS there), H * W < 2^25 (forward) and
 * B * Ho * Wo < 2^25 (input gradient): 32-bit byte offsets.  (Addition to ABI v24.)
 */
int64_t asr_conv7x7c32_workspace_bytes(void);
int asr_conv7x7c32_supported(int B, int H, int W, int stride_h);
int asr_conv7x7c32_fwd_bf16(const void *x, const float *w, int B, int H, int W, int stride_h,
                            void *y, double *chan_sums, void *workspace, int64_t workspace_bytes,
                            void *stream);
/* stride_h = 3 only (the shape the encoder uses); H, W are the INPUT's (dx's) extents */
int asr_conv7x7c32_bwd_data_bf16(const void *dy, const float *w, int B, int H, int W,
                                 int stride_h, void *dx, void *workspace,
                                 int64_t workspace_bytes, void *stream);
int asr_conv7x7c32_wgrad_bf16(const void *x, const void *dy, int B, int H, int W, int stride_h,
                              float *dw, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * The first convolution of the front-end, Conv2d(1, 32, (7, 7), stride (1, 2), padding (6, 0))
 * (reference deep_speech_2.py:52-66) on the raw one-channel features:
 *   x [B, T, F] f32, w [32, 1, 7, 7] f32, y [B, T + 6, (F - 7) / 2 + 1, 32] bf16 channels-last,
 *   bias-free; wgrad: dw [32, 1, 7, 7] f32 from x and dy (y's layout).  The input needs no
 *   gradient.  workspace: asr_conv1_7x7s2_workspace_bytes().
 */
int64_t asr_conv1_7x7s2_workspace_bytes(void);
int asr_conv1_7x7s2_fwd(const float *x, const float *w, int B, int T, int F, void *y,
                        double *chan_sums, void *workspace, int64_t workspace_bytes, void *stream);
int asr_conv1_7x7s2_wgrad(const float *x, const void *dy, int B, int T, int F, float *dw,
                          void *workspace, int64_t workspace_bytes, void *stream);
/*
 * The same weight gradient with the backward pass of the BatchNorm + Hardtanh behind the
 * convolution applied on the way in: dy is the gradient reaching the BatchNorm's OUTPUT, z the
 * convolution's saved output (both y's layout), and the kernel forms, per element, what phase 2
 * of asr_bn_act_bwd_phase_f32 would store as dx (same operations, same bits) without that
 * tensor ever existing.  conv_bias (or null), gamma, beta, save_mean, save_invstd, training,
 * lo, hi: as for asr_bn_act_bwd_phase_f32; bn_workspace: that call's workspace after its
 * phase 1 (the two per-channel sums, possibly all-reduced); n_total: the element count the
 * sums stand for.  asr_conv1_7x7s2_wgrad_bn_supported(F): 1 for the widths the fused kernel is
 * built for (the others return ASR_EUNSUPPORTED and keep the two-kernel path).
 * (Additions to ABI v24.)
 */
int asr_conv1_7x7s2_wgrad_bn_supported(int F);
int asr_conv1_7x7s2_wgrad_bn(const float *x, const void *z, const void *dy, int B, int T, int F,
                             const float *conv_bias, const float *gamma, const float *beta,
                             const float *save_mean, const float *save_invstd,
                             int training, float lo, float hi, const void *bn_workspace,
                             double n_total, float *dw, void *workspace,
                             int64_t workspace_bytes, void *stream);

/* The same first convolution for the WSJ recipes' real features: x [B, T, F, cin] f32 — the
 * reference's bs x t x f x c layout (deep_speech_2.py:127), cin = 3 (static, delta,
 * delta-delta; egs/wsj/yamls/ctc.yaml:8-15), F = 81 -> Fo = 38 — w [32, cin, 7, 7] f32, the
 * same outputs.  Built for cin == 3 and even Fo <= 48 (ASR_EUNSUPPORTED otherwise); workspace
 * asr_conv1c_7x7s2_workspace_bytes(cin).  (ABI v16) */
int64_t asr_conv1c_7x7s2_workspace_bytes(int cin);
/* asr_conv1_7x7s2_supported(F, cin): 1 if forward and weight gradient of the first convolution
 * both take F features of cin channels (the launchers run the same checks; with chan_sums the
 * forward entry points also need B * ceil((T + 6) / rows) <= 2^17 workgroups, rows = 16 for one
 * channel and 8 for three).  With Fo = (F - 7) / 2 + 1 that is Fo <= 39 for cin = 1 (F <= 84:
 * the weight gradient's LDS) and even Fo <= 40 for cin = 3 (F <= 86), 0 for every other cin.
 * (Addition to ABI v24.) */
int asr_conv1_7x7s2_supported(int F, int cin);
int asr_conv1c_7x7s2_fwd(const float *x, const float *w, int B, int T, int F, int cin, void *y,
                         double *chan_sums, void *workspace, int64_t workspace_bytes, void *stream);
int asr_conv1c_7x7s2_wgrad(const float *x, const void *dy, int B, int T, int F, int cin,
                           float *dw, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * One label step of the TCN / local-attention decoder for every live hypothesis
 * (replaces LocalAttention.forward, reference att_speech/modules/tcn.py:193-230, and the
 * context reduction of AttentionDecoderTCN.enc_step, :465-474).  Hypothesis h = u * beam + k
 * belongs to utterance u.
 *   eproj   [T, B, A]   encoded_to_hidden(encoded), per utterance, time-major
 *   enc     [T, B, E]   encoder output;  enc_lens [B]
 *   filt    [B*beam, A, Kf]  lm_to_kernel(lm_state) (Kf = 32 taps), glob [B*beam, A] lm_to_global(lm_state)
 *   w_score [A], b_score: hidden_to_score;  temperature: LocalAttention.temperature
 *   att_prev [B*beam, T] previous alignments, one row per hypothesis; parent [B*beam] (or
 *           null): hypothesis h continues row parent[h] (the beam's re-indexing, :551)
 *   att_new [B*beam, T]  softmax_t( w . tanh(eproj_t + (a_prev * filt)(t) + glob) * temperature + pad_t )
 *   context [B*beam, E]  sum_t att_new[t] enc[t]
 * Limits: Kf == 32, T <= 8160 (two alignment rows in 64 KiB of LDS; ASR_EUNSUPPORTED beyond).
 */
int asr_tcn_attention_step_f32(const float *eproj, const float *enc, const int32_t *enc_lens,
                               const float *filt, const float *glob, const float *w_score,
                               float b_score, float temperature,
                               const float *att_prev, const int32_t *parent,
                               int T, int B, int beam, int A, int Kf, int E,
                               float *att_new, float *context, void *stream);

/*
 * The same step under LocalAttention's force_forward = (win_lo, win_hi) (an addition to ABI
 * v24; replaces recompute_forward_mask, reference att_speech/modules/tcn.py:165-188, and its
 * use in LocalAttention.forward, :226-228, together with what the entry above replaces).
 * Operands as above, plus the window.  With a = att_prev[parent[h]] (att_prev[h] when parent
 * is null):
 *   peak  = max_t a[t] over all T frames, where = the LOWEST t that attains it (ties go to the
 *           first maximum, as torch.max over a row gives them)
 *   active = peak >= 0.1f  (the reference's `att_max.item() < 0.1` negated; no fp32 value lies
 *           between 0.1 and 0.1f)
 *   mask_t = (t >= enc_lens[u] ? -1e5 : 0)
 *          + (active && (t < where + win_lo || t >= where + win_hi) ? -1e5 : 0)
 *   att_new = softmax_t( (w . tanh(...) + b) * temperature + mask_t ),  context as above.
 * A frame that is both padded and outside the window carries -2e5.  Only the frames with the
 * fewest masks can get a weight (exp(-1e5 + O(100)) is an exact zero in every format): the
 * kernel evaluates scores and context on those frames alone and writes an exact 0.0f to every
 * other frame of att_new.  A window clipped to nothing, or lying wholly at or behind enc_lens,
 * leaves the softmax over frames that all carry one -1e5 (two, when enc_lens is 0 as well); a
 * diffuse row (peak < 0.1f) is treated as by the entry above.
 * Limits: those of the entry above; win_lo >= win_hi or win_hi < 1 is ASR_EUNSUPPORTED (with
 * win_hi < 1 the reference's `mask[right:]` takes a negative slice index and means something
 * else).
 */
int asr_tcn_attention_step_win_f32(const float *eproj, const float *enc, const int32_t *enc_lens,
                                   const float *filt, const float *glob, const float *w_score,
                                   float b_score, float temperature,
                                   const float *att_prev, const int32_t *parent,
                                   int T, int B, int beam, int A, int Kf, int E,
                                   int win_lo, int win_hi,
                                   float *att_new, float *context, void *stream);

/*
 * The training recurrence of the same local attention over all label positions (ABI v24;
 * replaces the per-position loop of AttentionDecoderTCN.forward, reference
 * att_speech/modules/tcn.py:357-440, over LocalAttention.scores / forward, :190-230, and the
 * backward pass autograd replays through it).  One workgroup per utterance for the whole scan.
 *   eproj  [T, B, A]     encoded_to_hidden(encoded), time-major
 *   filt   [L, B, A*Kf]  lm_to_kernel(lm_states): the Kf = 32 taps of one unit contiguous
 *   glob   [L, B, A]     lm_to_global(lm_states)
 *   a0     [T, B]        the initial alignment a_{-1} (init_attention)
 *   w_score [A], b_score [1] (device memory): hidden_to_score;  enc_lens [B] int32
 *   fwd: att [L, B, T]   a_l = softmax_t( temperature * (w . tanh(eproj_t + glob_l +
 *                        sum_j a_{l-1}[t-(Kf-1)+j] filt_l[., j]) + b) + pad_t ), the previous
 *                        alignment left-padded with zeros; pad_t = -1e5 for t >= enc_lens[b]
 *   bwd: d_att [L, B, T] the gradient reaching each a_l from outside the recurrence; the
 *                        gradients of the inputs: d_eproj [T, B, A], d_filt [L, B, A*Kf],
 *                        d_glob [L, B, A], d_a0 [T, B], and per-utterance partials
 *                        d_wb [B, A+1] of d w_score (A entries) and d b_score (the last one;
 *                        zero up to rounding, the softmax being shift-invariant).
 * h is recomputed in the backward pass; nothing but att is saved.  Every reduction has a
 * fixed owner and order: the results are bitwise reproducible.  Limits: Kf == 32,
 * 1 <= A <= 256, 1 <= T <= 4096 (ASR_EUNSUPPORTED beyond), L >= 1, B >= 1.
 */
int asr_tcn_attention_scan_fwd_f32(const float *eproj, const float *filt, const float *glob,
                                   const float *a0, const float *w_score, const float *b_score,
                                   float temperature, const int32_t *enc_lens, int T, int B,
                                   int L, int A, int Kf, float *att, void *stream);
int asr_tcn_attention_scan_bwd_f32(const float *eproj, const float *filt, const float *glob,
                                   const float *a0, const float *w_score, float temperature,
                                   const int32_t *enc_lens, const float *att, const float *d_att,
                                   int T, int B, int L, int A, int Kf, float *d_eproj,
                                   float *d_filt, float *d_glob, float *d_a0, float *d_wb,
                                   void *stream);

/*
 * The label scan of the RNN attention decoder (an addition to ABI v24; replaces the
 * per-position loop of AttentionDecoderRNN.forward, reference att_speech/modules/decoders/
 * attention_decoder.py:217-232 over Attention.forward :90-111, one nn.GRU step per position,
 * and, with L = 1, one label step of .decode :324-337).  Per hypothesis b and position l:
 *   rec_l = w_rec h_{l-1}
 *   a_l   = softmax_t( w_score . tanh(eproj_t + rec_l) + b_score + pad_t ),
 *           pad_t = -1e5 for t >= enc_lens: those frames get exactly 0
 *   c_l   = sum_t a_l[t] encoded_t
 *   gi = gx_emb_l + w_ic c_l,  gh = w_hh h_{l-1} + b_hh            (gate order r, z, n)
 *   r = σ(gi_r + gh_r)  z = σ(gi_z + gh_z)  n = tanh(gi_n + r ⊙ gh_n)  h_l = (1−z) ⊙ n + z ⊙ h_{l-1}
 * One workgroup per hypothesis for the whole scan; fp32 throughout.
 *   eproj   [T, B/beam, A]  encoded_to_hidden(encoded) (bias included), time-major
 *   encoded [T, B/beam, E];  enc_lens [B/beam] int32: hypothesis b reads utterance b / beam
 *   gx_emb  [L, B, 3H]      embedding half of W_ih x + b_ih (b_ih included)
 *   w_ic [3H, E] context half of W_ih;  w_hh [3H, H];  b_hh [3H];  w_rec [A, H]
 *   w_score [A], b_score [1] (device memory);  h0 [B, H]
 *   fwd out: att [L, B, T], states [L, B, H]; for the backward pass (each may be null):
 *            contexts [L, B, E], gates [L, B, 4H] = one record (r, z, n, gh_n) per unit,
 *            rec [L, B, A]
 *   bwd (beam = 1): w_icT [E, 3H], w_hhT [H, 3H], w_recT [H, A] are the transposes;
 *            d_att [L, B, T] and d_states [L, B, H] are the gradients reaching the outputs
 *            from outside the recurrence (either may be null = zero).  Written:
 *            d_eproj [T, B, A]   ACCUMULATED: the caller zero-fills it
 *            d_gates [L, B, 4H]  (dr, dz, dn, dn ⊙ r) pre-activation gradients: the first 3H
 *                                are d gx_emb and the operand of d w_ic (with contexts); dr,
 *                                dz, dn ⊙ r are d b_hh's terms and the operand of d w_hh
 *                                (with h_{l-1})
 *            d_contexts [L, B, E]  operand of d encoded = sum_l a_l ⊗ d c_l
 *            d_rec [L, B, A]     operand of d w_rec (with h_{l-1})
 *            d_w_score [B, A]    per-hypothesis partials of d w_score (d b_score is zero:
 *                                the softmax is shift-invariant)
 *            d_h0 [B, H]
 * The alignment itself is not carried from position to position (only the reference's
 * force_forward window reads the previous one; that option stays outside these kernels), so
 * there is no initial-alignment operand.  Every reduction has a fixed owner and order: the
 * results are bitwise reproducible.  Limits: 1 <= T <= 4096, A <= 320, H <= 320, E <= 512,
 * A, E and H multiples of 4 (ASR_EUNSUPPORTED beyond); L >= 1, B >= 1, beam >= 1 dividing B.
 */
int asr_att_gru_scan_fwd_f32(const float *eproj, const float *encoded, const int32_t *enc_lens,
                             const float *gx_emb, const float *w_ic, const float *w_hh,
                             const float *b_hh, const float *w_rec, const float *w_score,
                             const float *b_score, const float *h0, int T, int B, int beam,
                             int L, int A, int E, int H, float *att, float *states,
                             float *contexts, float *gates, float *rec, void *stream);
int asr_att_gru_scan_bwd_f32(const float *eproj, const float *encoded, const int32_t *enc_lens,
                             const float *w_icT, const float *w_hhT, const float *w_recT,
                             const float *w_score, const float *h0, const float *att,
                             const float *states, const float *gates, const float *rec,
                             const float *d_att, const float *d_states, int T, int B, int L,
                             int A, int E, int H, float *d_eproj, float *d_gates,
                             float *d_contexts, float *d_rec, float *d_w_score, float *d_h0,
                             void *stream);

/*
 * One step of BeamSearch for every utterance, without a host read-back (replaces
 * BeamSearch.step + _save_best_finished, reference att_speech/modules/beam_search.py:58-124,
 * 147-175).  logits [B*beam, C] (class C-1 = EOS); scores_in / scores_out [B*beam] running
 * scores (distinct buffers); est_in / est_out [B*beam, Lcap] label histories (distinct
 * buffers, `step` labels each on entry); len_div = step ** length_normalization.
 * Per utterance: finished_count [B], best_score [B] (init -inf; the RAW EOS score, the
 * reference's aliasing quirk), best_len [B], best_tokens [B, Lcap].  Outputs new_input
 * [B*beam] (chosen labels), parent [B*beam] (flat index of the hypothesis each survivor
 * extends).  done_and_scratch [3] int32, zero before the first step: word 0 becomes 1 after
 * the step in which every utterance reached finished_count >= beam; calls with the flag set
 * change nothing, so a host polling it every few steps sees the reference's results; word 2
 * counts the steps that took effect (the final histories are in the buffer written by the
 * last of them), word 1 is scratch.
 * Ties: the top-k is a stable descending sort of the candidates beam * (C-1) + class, so equal
 * scores go to the lower candidate index, -inf ones included (they fill the slots the finite
 * candidates leave; with fewer candidates than beams the rest are -inf copies of the last sorted
 * index); EOS must be strictly above every other class of its row to count as best, and a row
 * whose running score is -inf never does; among beams with equal normalised EOS scores the first
 * wins; a best_score equal to the candidate stays.  beam <= 32, beam * (C-1) <= 2048
 * (ASR_EUNSUPPORTED beyond); Lcap > step (ASR_EINVAL).
 */
int asr_beam_step_f32(const float *logits, const float *scores_in, float *scores_out,
                      const int32_t *est_in, int32_t *est_out, int step, int B, int beam, int C,
                      int Lcap, float len_div, int32_t *finished_count, float *best_score,
                      int32_t *best_len, int32_t *best_tokens, int32_t *new_input,
                      int32_t *parent, int32_t *done_and_scratch, void *stream);

/*
 * The LM-fused beam search (BeamSearchLM, reference att_speech/modules/beam_search.py:185-363) on
 * the device, for any number of utterances; additions to ABI v24.  A batch of B utterances behaves
 * as B independent BeamSearchLM(batch_size = 1) runs, each on its own enc_lens[b] frames.
 *
 * The LM is the CSR bundle of att_speech.lm_fst.LmFst: ptr [S+1] (arcs of s are [ptr[s], ptr[s+1]),
 * ilabel-sorted, so its epsilon arcs are [ptr[s], ptr_ne[s])), dst / ilabel [A] int32, weight [A]
 * fp64 (costs, -log p), rank [S] = eps_rank() (every epsilon arc climbs in rank; max_rank its
 * maximum), and arc_w_closed [A] = weight[a] - log Z(dst[a]) with Z(n) the total weight of all
 * epsilon paths out of n, the empty one included.  mapping [C]: LM label of every class.
 * A hypothesis carries a bag of at most ASR_LM_BAG_CAP entries: bag_state [hyps, cap] int32 in
 * ascending state order, bag_cost [hyps, cap] fp64, bag_n [hyps]; bag_cap must be ASR_LM_BAG_CAP
 * (ASR_EUNSUPPORTED otherwise).
 *
 * asr_lm_label_costs_f64: cost [hyps, C] fp64, cost[h, c] = -log sum over the entries (s, w) of
 * bag h and the arcs a of s with ilabel mapping[c] of exp(-(w + arc_w_closed[a])), +inf where there
 * is no such arc: the cost of the epsilon-closed bag of the extension, without building it.
 * Summed in the order (entry, arc).  frozen [B] (may be NULL): rows of utterances with frozen[b] != 0
 * are left alone.
 *
 * asr_beam_lm_step_f32: one BeamSearchLM.step per utterance, one workgroup each, no read-back.
 * logits [hyps, C] (class C-1 = EOS), att [hyps, T] this step's alignment, lm_cost as above (NULL:
 * no LM term, lm_weight == 0).  total = acoustic + (float)(-lm_weight * min(1e20, lm_cost))
 * (+ coverage_weight * #{t < len : cov_in + att > coverage_tau} when coverage_weight > 0); only the
 * acoustic part is carried in scores_in / scores_out [hyps].  min_eos [hyps] (NULL: keep_eos_score
 * off; init -inf): the EOS logit is raised to it before the log-softmax and it is re-indexed in
 * place.  est_in / est_out [hyps, Lcap], cov_in / cov_out [hyps, T] (init 0; may be NULL when
 * coverage_weight <= 0) are distinct buffers that the caller alternates.  From step 1 on a
 * hypothesis finishes when EOS is strictly the best class of its total row, the peak of its
 * alignment (first maximum over t < len) is > min_attention_pos * len, and total[EOS] / len_div is
 * > -1e10.  The finished list is double-buffered by fin_parity [B] (0 / 1, flipped by a step that
 * adds): fin_score / fin_len / fin_beam [2, B, beam], fin_tokens [2, B, beam, Lcap], fin_count [B];
 * sorted descending and stable (older entries first), cut to beam.  In a step that added, on a
 * strict improvement over best_score [B] (init -inf): best_len, best_tokens [B, Lcap] and
 * best_elems [B, 3] = {acoustic, lm, coverage} of THIS step's EOS column at the beam index stored
 * with entry 0 (the reference's quirk; the third element is left alone when coverage_weight <= 0).  The top-k runs on total over beam * (C-1) + class
 * (first step: beam 0 only; lowest index wins ties; -inf candidates fill up in index order; with
 * fewer candidates than beams the last sorted index is repeated), slots r >= ncand get score -inf,
 * and when beam == ncand EVERY slot does (the reference's slice `[-0:]`).  Outputs new_input /
 * parent [hyps].  nsteps [B] = step + 1 for every utterance the launch worked on; frozen [B]
 * (init 0) is set after the step that filled the finished list, and launches change nothing of a
 * frozen utterance.  Limits as asr_beam_step_f32: beam <= 32, beam * (C-1) <= 2048.
 *
 * asr_lm_bag_advance_f64: the bags of the survivors of that step (utterances with nsteps[b] ==
 * step + 1): from the bag of parent[h], the arcs with ilabel mapping[new_input[h]] (plain weight),
 * equal targets merged, closed over the epsilon arcs level by level in rank order.  in_* and out_*
 * are distinct buffers.  A bag that asks for more than bag_cap entries is cut and raises
 * *overflow (int32, init 0) to the size it asked for (an integer max; a lower bound once entries
 * are dropped): the caller discards the search.
 *
 * Every sum has a fixed owner and order: launches are reproducible bit for bit.
 */
#define ASR_LM_BAG_CAP 32
int asr_beam_lm_supported(int beam, int C, int bag_cap);
int asr_lm_label_costs_f64(const int32_t *ptr, const int32_t *ilabel, const double *arc_w_closed,
                           int nstates, const int32_t *bag_state, const double *bag_cost,
                           const int32_t *bag_n, int bag_cap, const int32_t *mapping,
                           const int32_t *frozen, int B, int beam, int C, double *cost, void *stream);
int asr_lm_bag_advance_f64(const int32_t *ptr, const int32_t *ptr_ne, const int32_t *dst,
                           const int32_t *ilabel, const double *weight, const int32_t *rank,
                           int nstates, int max_rank, const int32_t *mapping,
                           const int32_t *in_state, const double *in_cost, const int32_t *in_n,
                           int32_t *out_state, double *out_cost, int32_t *out_n, int bag_cap,
                           const int32_t *parent, const int32_t *new_input, const int32_t *nsteps,
                           int step, int B, int beam, int32_t *overflow, void *stream);
int asr_beam_lm_step_f32(const float *logits, const float *att, const int32_t *enc_lens,
                         const double *lm_cost, double lm_weight, const float *scores_in,
                         float *scores_out, const int32_t *est_in, int32_t *est_out,
                         const float *cov_in, float *cov_out, float *min_eos, int step, int B,
                         int beam, int C, int T, int Lcap, float len_div, double min_attention_pos,
                         float coverage_tau, float coverage_weight, int32_t *fin_count,
                         int32_t *fin_parity, float *fin_score, int32_t *fin_len, int32_t *fin_beam,
                         int32_t *fin_tokens, float *best_score, int32_t *best_len,
                         int32_t *best_tokens, float *best_elems, int32_t *new_input,
                         int32_t *parent, int32_t *frozen, int32_t *nsteps, void *stream);

/*
 * The graph search (GraphSearch, reference att_speech/modules/beam_search.py:406-648: BeamSearchLM
 * that merges hypotheses whose recent history, LM-state set and attention agree) on the device;
 * additions to ABI v24.  Per label step: asr_lm_label_costs_f64, asr_beam_lm_step_graph_f32,
 * asr_lm_bag_advance_f64, asr_graph_merge_f32.
 *
 * asr_beam_lm_step_graph_f32: asr_beam_lm_step_f32 (the same kernel; every shared output bit for
 * bit) with two more outputs.  fin_mask [hyps] int32: 1 where this step's finish test passed for
 * that OLD beam slot, else 0; all 0 at step 0; left alone for frozen utterances.  tot_out [hyps]:
 * the fused score (EOS ignored) of the chosen (beam, class) pair per NEW slot, with the same -inf
 * padding rule as scores_out (the host's new_tot_scores).  tot_out is a buffer of its own.
 *
 * asr_graph_merge_f32: the two host loops of GraphSearch.step (reference :466-476 and :518-590),
 * one workgroup of 256 threads per utterance, for the utterances with nsteps[b] == step + 1;
 * launched after asr_lm_bag_advance_f64, because it reads the survivors' new bags.
 * att [hyps, T] is this step's alignment as the step entry saw it (NOT re-indexed by parent),
 * scores / tot [hyps] are scores_out / tot_out of the step entry (both modified), est_in / est_out
 * the histories before / after the step, bag_state [hyps, bag_cap] / bag_n [hyps] the survivors'
 * bags (both NULL: no LM term, the LM-state test is skipped and nodes carry an empty set),
 * len_pow [Lcap + 1] fp32 with len_pow[l] = (float)(l ** length_normalization) filled by the host.
 * The node store is the caller's, Ncap >= (step + 1) * beam nodes per utterance (every live slot of
 * every step appends at most one node, so it cannot overflow; ASR_EINVAL otherwise), node index =
 * insertion order: node_count [B] (init 0), node_score [B, Ncap] fp32, node_len [B, Ncap],
 * node_tokens [B, Ncap, Lcap], node_att [B, Ncap, T] fp32, node_bag_n [B, Ncap], node_bag_state
 * [B, Ncap, bag_cap], node_fin [B, Ncap], node_uplink [B, Ncap] (-1: none, else a node index of the
 * same utterance).  Semantics, the host class's, quirks included:
 *  - bucket: the nodes whose last `span` labels, left-filled with -1, are equal (span 0: one bucket
 *    for all).  Labels are compared directly; collisions of Python's hash() between different
 *    tuples, which would join buckets on the host, are not reproduced.
 *  - finished marks come first: for every old slot with fin_mask set, every node whose label
 *    sequence equals that slot's history in est_in (length step) gets fin = 1.
 *  - the new slots are walked in order cur = 0 .. beam-1, each seeing what the earlier ones did
 *    (appended nodes, uplinks, scores set to -inf); a slot whose scores[cur] is -inf is skipped and
 *    appends nothing.
 *  - candidates are the bucket's nodes in insertion order; one is skipped when it has an uplink,
 *    when there is an LM term and its LM-state array differs from the slot's new bag states, or
 *    when sum over t < enc_lens[b] of min(node_att[t], att[cur][t]) < merge_threshold.
 *  - the alignment column is the one at the NEW slot index cur of this step's alignment, before
 *    re-indexing by parent (the reference's att_weights[:, current_id]), not the parent's.
 *  - score test in fp32: node_score / len_pow[node_len] >= tot[cur] / len_pow[step + 1].  True
 *    (ties included), the old branch wins: scores[cur] = tot[cur] = -inf, the slot's uplink is that
 *    candidate, the walk over candidates ends.  False, the new branch wins: the candidate's uplink
 *    becomes the index the new node is about to get, every OTHER new slot whose history has the
 *    candidate's sequence as a prefix gets -inf in both scores, and the walk goes on.
 *  - then the node is appended: tot[cur] as it is now, the alignment column, the bag's states,
 *    fin = 0, the history from est_out (length step + 1), the uplink.
 *  - alias: the host stores a VIEW of new_tot_scores[cur], so when a later slot of the same step
 *    drops slot cur, the node appended for cur in this step reads -inf from then on, also in the
 *    score tests of that step.
 *  - scores leaves the launch with the -inf entries (the host's self.scores = new_scores).
 * No floating-point atomics; every sum has one owner and a fixed order (per-lane partial sums in
 * frame order, then a fixed shuffle tree): launches are reproducible bit for bit.
 * asr_graph_search_supported: beam <= 32, span >= 0, 1 <= T <= 8160, bag_cap == ASR_LM_BAG_CAP.
 */
int asr_graph_search_supported(int beam, int span, int T, int bag_cap);
int asr_beam_lm_step_graph_f32(const float *logits, const float *att, const int32_t *enc_lens,
                               const double *lm_cost, double lm_weight, const float *scores_in,
                               float *scores_out, const int32_t *est_in, int32_t *est_out,
                               const float *cov_in, float *cov_out, float *min_eos, int step, int B,
                               int beam, int C, int T, int Lcap, float len_div,
                               double min_attention_pos, float coverage_tau, float coverage_weight,
                               int32_t *fin_count, int32_t *fin_parity, float *fin_score,
                               int32_t *fin_len, int32_t *fin_beam, int32_t *fin_tokens,
                               float *best_score, int32_t *best_len, int32_t *best_tokens,
                               float *best_elems, int32_t *new_input, int32_t *parent,
                               int32_t *frozen, int32_t *nsteps, int32_t *fin_mask, float *tot_out,
                               void *stream);
int asr_graph_merge_f32(const float *att, const int32_t *enc_lens, float *scores, float *tot,
                        const int32_t *est_in, const int32_t *est_out, const int32_t *fin_mask,
                        const int32_t *bag_state, const int32_t *bag_n, int bag_cap,
                        const int32_t *nsteps, const float *len_pow, int step, int B, int beam, int T,
                        int Lcap, int span, float merge_threshold, int Ncap, int32_t *node_count,
                        float *node_score, int32_t *node_len, int32_t *node_tokens, float *node_att,
                        int32_t *node_bag_n, int32_t *node_bag_state, int32_t *node_fin,
                        int32_t *node_uplink, void *stream);

/*
 * Forced scoring of given sentences through their prefix trie (the teacher-forced pass of the
 * reference's egs/wsj/local/lattice_search/rescore_lattices2.py and score_groundtruth.py,
 * score_acoustic); an addition to ABI v24.  The sentences of an utterance, EOS appended, form a
 * trie; the distinct prefixes of length l are the UNITS of level l, and one level is one label step
 * of the decoder for all of them (asr_tcn_attention_step_f32 with parent = the unit extended).
 *
 * asr_forced_level_f32: the bookkeeping of one trie level, one workgroup of 256 threads per unit
 * slot, no read-back.  B utterances with `width` slots each: slot p belongs to utterance p / width.
 * logits [B * width, C] (class C-1 = EOS) and att [B * width, T] are this step's outputs per slot.
 *  - cov_out[p, t] = cov_in[parent[p], t] + att[p, t] for t < T (one fp32 add).  cov_in has
 *    cov_in_rows rows (the previous level's slots; at level 0 the initial alignments, which the
 *    reference's coverage includes) and parent [B * width] indexes them; cov_in and cov_out are
 *    distinct buffers that the caller alternates.
 *  - The outgoing edges of slot p are edge_ptr[p] .. edge_ptr[p + 1] (edge_ptr [B * width + 1],
 *    ascending, <= n_edges) of edge_label / edge_dst [n_edges].  With m = max_c logits[p, c] and
 *    ls = log sum_c exp(logits[p, c] - m), edge e carries
 *        v = acoustic_in[p] + (double)((logits[p, edge_label[e]] - m) - ls):
 *    fp32 terms (log_softmax(logits)[label]) in an fp64 running sum, the reference's sum() of .item()
 *    values.  edge_dst[e] >= 0: a slot of the NEXT level, acoustic_out[edge_dst[e]] = v
 *    (acoustic_out [n_out]; acoustic_in [B * width] is all 0 at level 0; distinct buffers).
 *    edge_dst[e] < 0: the EOS edge of sentence s = -1 - edge_dst[e] (< n_sent), sent_acoustic[s] = v
 *    and sent_covered[s] = #{t < enc_lens[p / width] : cov_out[p, t] > coverage_tau} (int32, counted
 *    once per slot).  Every destination has exactly one edge in the whole trie.
 *  - A slot without edges (edge_ptr[p] == edge_ptr[p + 1]) is dead: it writes its cov_out row and
 *    nothing else.  Edges whose label, destination or sentence is out of range are skipped.
 * The class sum runs per lane over c = lane, lane + 64, ... and through the xor-shuffle tree, the
 * count per thread over t = tid, tid + 256, ..., the tree, then waves 0..3: launches are
 * reproducible bit for bit, there is no atomic.  Limits (the step kernel's): 2 <= C <= 2048,
 * 1 <= T <= 8160, ASR_EUNSUPPORTED beyond; NULL or aliased buffers ASR_EINVAL, before any launch.
 */
int asr_forced_level_f32(const float *logits, const float *att, const float *cov_in, float *cov_out,
                         const int32_t *parent, const int32_t *edge_ptr, const int32_t *edge_label,
                         const int32_t *edge_dst, const double *acoustic_in, double *acoustic_out,
                         const int32_t *enc_lens, int B, int width, int C, int T, int cov_in_rows,
                         int n_edges, int n_out, int n_sent, float coverage_tau,
                         double *sent_acoustic, int32_t *sent_covered, void *stream);

/*
 * The step boundary on the device (ABI v18): the reference's GradientClipping hook
 * (att_speech/modules/hooks/gradient_clipping.py:13-53: clip_grad_norm_ to clip_norm, skip the
 * optimizer step when the unclipped norm exceeds skip_step_norm) and torch.optim.Adam.step
 * (trainer.py:262-266; amsgrad / maximize off, weight_decay as L2) without a host read-back
 * between backward and the update.
 *
 * asr_grad_sumsq_partials_f32: partials[i] = sum of g^2 over the i-th of nparts equal slices of
 * the flat gradient g [n] (nparts <= 65535).
 * asr_adam_clip_step_f32: norm = sqrt(sum partials); the step is skipped when norm >
 * skip_norm, when it is not finite, or when *err_word != 0 (the persistent LSTM's error word,
 * may be NULL); otherwise g is scaled by min(1, clip_norm / (norm + 1e-6)) and Adam step number
 * *step_in + 1 updates m_flat / v_flat [n] and the parameters.  The parameters stay where the
 * caller's framework allocated them: `chunks` (device memory, nchunks entries)
 * lists pieces of at most asr_adam_chunk_elems() elements: `param` = address of the piece
 * inside its parameter tensor, `flat_offset` = its offset in g / m / v.  *step_out = *step_in + 1
 * (or *step_in when skipped); step_in != step_out (the caller alternates two words).
 * stats [4] = {norm, clipped, skipped, err} as floats, for the host to read when it likes.
 */
/*
 * asr_lattice_fwbw_f32 with the occupancies written times grad_sign (+1 or -1) (ABI v20): a
 * decoder that needs -logZ (the numerator of FSTDecoder.get_fst_loss, advanced_decoder.py:486-496)
 * asks for -1 and receives the gradient of what it uses; the backward pass of PathLogSumExp
 * (fst_utils.py:482-485: grad_output[None, :, None] * grads) then multiplies by +1 —
 * asr_scale_rows_f32 (x [T,B,C] *= scale [B] in place) leaves utterances whose factor is exactly 1
 * untouched, so the usual backward pass makes no pass over the [T,B,C] tensor at all (1.6 GB at
 * C = 2401, 512 utterances).  out_logZ is +logZ either way.
 */
int asr_lattice_fwbw_signed_f32(const float *lp, int T, int B, int C, const int32_t *lens,
                                const int32_t *src_in, const int32_t *il_in, const float *w_in,
                                const float *term, const int32_t *dst_out, const int32_t *il_out,
                                const float *w_out, int N, int Kin, int Kout, int Bg, float neg_inf,
                                float grad_sign, float *out_logZ, float *out_grad,
                                float *out_logZ_bwd, void *workspace, int64_t workspace_bytes,
                                void *stream);
int asr_scale_rows_f32(float *x, int T, int B, int C, const float *scale, void *stream);

typedef struct AsrAdamChunk {
    void *param;
    uint32_t flat_offset;
    uint32_t count;
} AsrAdamChunk;
int asr_adam_chunk_elems(void);
int asr_grad_sumsq_partials_f32(const float *g, int64_t n, float *partials, int nparts, void *stream);
int asr_adam_clip_step_f32(const AsrAdamChunk *chunks, int nchunks, const float *g_flat,
                           float *m_flat, float *v_flat, const float *partials, int nparts,
                           const uint32_t *err_word, float lr, float beta1, float beta2, float eps,
                           float weight_decay, float clip_norm, float skip_norm,
                           const int32_t *step_in, int32_t *step_out, float *stats, void *stream);

/*
 * asr_adam_clip_step_f32 with one more skip request (ABI v23): the reference's KillOnNan hook
 * (att_speech/modules/hooks/kill_on_nan.py:14-27, a `loss.item()` per step that asks the trainer,
 * trainer.py:241-248, to skip the optimizer step when the loss is NaN or +-inf) decided on the
 * device.  skip_word (may be NULL) != 0 skips the step, OR-ed with the norm / non-finite norm /
 * err_word rules; stats [5] = {norm, clipped, skipped, err, skip_word != 0} when skip_word is
 * given (stats [4] as before when it is NULL).  asr_adam_clip_step_f32 is this entry with
 * skip_word = NULL, bit for bit.
 */
int asr_adam_clip_step_ex_f32(const AsrAdamChunk *chunks, int nchunks, const float *g_flat,
                              float *m_flat, float *v_flat, const float *partials, int nparts,
                              const uint32_t *err_word, float lr, float beta1, float beta2, float eps,
                              float weight_decay, float clip_norm, float skip_norm,
                              const int32_t *step_in, int32_t *step_out, const uint32_t *skip_word,
                              float *stats, void *stream);

/*
 * The loss test of KillOnNan (kill_on_nan.py:16-22: `torch.isnan(loss).item()`, `loss.item() ==
 * INF or loss.item() == MINF`) without the read-back (ABI v23): *flag = 1 when any of x [n] is
 * NaN or +-inf, 0 otherwise; one single-workgroup launch, meant for the loss (n small).  The flag
 * feeds asr_adam_clip_step_ex_f32's skip_word.
 */
int asr_nonfinite_flag_f32(const float *x, int n, uint32_t *flag, void *stream);

/*
 * Counter-based Gaussian noise (ABI v23): the reference's weight noise
 * (att_speech/modules/hooks/weight_noise.py:63-99: `randn_like(weight) * sigma` added before the
 * forward pass, the stored tensor subtracted after backward) and ConstantGradientNoise
 * (gradient_noise.py:10-16: `grad += randn_like(grad) * sigma`) as one launch over a table of
 * pieces, with nothing stored between the two passes.
 *
 * segs (device memory, nsegs entries): `data` = address of a piece of fp32 memory, `index` = the
 * global noise index of its first element (index + count < 2^34), `count` <= asr_noise_chunk_elems(),
 * `sigma`.  z[i] for global index i is Philox4x32-10 with key = (seed lo, seed hi) and counter =
 * (i >> 2, tag, iteration lo, iteration hi); its four output words x0..x3 give
 * z[4g], z[4g+1] from (x0, x1) and z[4g+2], z[4g+3] from (x2, x3) by Box-Muller:
 * u = (x >> 9) * 2^-23 + 2^-24, r = sqrtf(-2 logf(u_a)), (s, c) = sincospif(2 u_b),
 * z_a = r c, z_b = r s.  z depends on (seed, tag, iteration, i) only: not on addresses, the
 * launch shape or the process.
 *   mode ASR_NOISE_APPLY: data[k] = data[k] + sign * (sigma * z) with sign = +1 or -1, product and
 *                         sum each rounded once (no FMA): apply(+1) then apply(-1) is
 *                         `w.add_(rand); w.add_(-rand)` with rand = sigma * z in fp32;
 *   mode ASR_NOISE_WRITE: data[k] = z (sigma and sign unused).
 * tag 0 is weight noise, tag 1 gradient noise.
 */
typedef struct AsrNoiseSegment {
    void *data;
    uint64_t index;
    uint32_t count;
    float sigma;
} AsrNoiseSegment;
#define ASR_NOISE_APPLY 0
#define ASR_NOISE_WRITE 1
int asr_noise_chunk_elems(void);
int asr_gaussian_noise_f32(const AsrNoiseSegment *segs, int nsegs, uint64_t seed, uint32_t tag,
                           uint64_t iteration, int mode, int sign, void *stream);

/*
 * Batched Levenshtein distance with operation counts: the scoring of do_evaluate
 * (att_speech/utils.py:35-65 `edit_distance_with_stats(x, y)`, called twice per utterance at
 * utils.py:324-327, x = the hypothesis, y = the reference text).  These entry points are additions:
 * no existing signature changes, so the ABI version stays 24.
 *
 * x, y: the token ids of all pairs, flat; pair p is x[x_off[p] : x_off[p+1]] against
 * y[y_off[p] : y_off[p+1]] (x_off, y_off: n_pairs + 1 prefix offsets).  out [n_pairs, 4] =
 * (dist, ins, del, sub) per pair.  dp[i][0] = i, dp[0][j] = j; a cell takes the minimum of
 * (dp[i-1][j] + 1 "ins", dp[i][j-1] + 1 "del", dp[i-1][j-1] + (x != y) "sub") and the FIRST minimum
 * in that order wins (np.argmin); the counts are those of the reference's trace-back along the
 * chosen moves, a move counting only where the distance grows.  They are carried forward with the
 * distance from the chosen predecessor (the same path read the other way), so no operation matrix
 * is kept.  All results are exact integers; dist == ins + del + sub.
 *
 * max_x, max_y: upper bounds (host values) of the pairs' lengths; they size the launch.  A pair
 * longer than the bounds it was launched with, or with decreasing offsets, gets (-1, -1, -1, -1).
 * ASR_EINVAL before anything is launched: null pointers with n_pairs > 0, negative counts, or
 * max_x / max_y above asr_edit_distance_max_len() (4096).  One wave per pair, no workspace, no
 * atomics.
 */
int asr_edit_distance_max_len(void);
int asr_edit_distance_stats_i32(const int32_t *x, const int32_t *x_off, const int32_t *y,
                                const int32_t *y_off, int n_pairs, int max_x, int max_y,
                                int32_t *out, void *stream);

/*
 * Forward-backward / alpha scan over ONE weighted sparse graph shared by the batch, in CSR
 * form (csrc/lattice_shared.hip): the decoding graph HC o G the reference builds when a
 * grammar FST is given (get_decoding_fst, fst_utils.py:633-640) — the denominator of the
 * globally normalised loss (advanced_decoder.py:497-505) and the search graph of
 * FSTDecoder.decode (:536-593).  Same results as asr_lattice_fwbw_f32 /
 * asr_lattice_forward_f32 (PathLogSumExp.forward fst_utils.py:400-488; path_reduction's alpha
 * scan :349-397 with the viterbi branch :366-370) on the padded [1,N,K] matrices of the same
 * graph, up to fp32 summation order; the start state is 0.  These entry points are additions:
 * no existing signature changes, so the ABI version stays 24.
 *
 *   N, E                  states and arcs (epsilon-free; parallel arcs already merged)
 *   in_ptr  [N+1] i32     in-arcs of state n are in_arc[in_ptr[n] .. in_ptr[n+1]), sorted by
 *                         (source, ilabel, weight) like the rows of fst_to_matrices (:285)
 *   in_arc  [E,2] u32     word 0 = source state | ilabel << 16, word 1 = the f32 weight's bits
 *   out_ptr / out_arc     the same arcs by source state, word 0 = destination | ilabel << 16
 *   term    [N]   f32     terminal log-weights (neg_inf where not final)
 *   order_in  [N] i32     the states in the order the scan takes them: the first n_light_in are
 *                         reduced by lanes_in (1..64, a power of two) adjacent lanes each, the
 *                         rest (high in-degree) by a whole wave each.  order_out / n_light_out
 *                         / lanes_out: the same for the beta scan over the out-arcs.
 *   grad_sign   +1, or -1 for the occupancies of -logZ (as asr_lattice_fwbw_signed_f32)
 *   accumulate  != 0: out_grad += occupancies, rows past an utterance's end left as they are
 *               (as asr_lattice_grouped_fwbw_acc_f32)
 *   out_best_il ties pick the first maximum in in-arc order; rows t >= lens[b] are 0
 *   workspace: asr_lattice_shared_workspace_bytes(T,B,N) bytes (fwbw always; forward only with
 *              viterbi != 0 and out_best_il != NULL)
 * lens[b] == 0 gives logZ = term[0] and an all-zero gradient.  The caller guarantees every
 * state index < N, every ilabel < C and every in-degree <= 65535.
 * asr_lattice_shared_supported: N <= 7168 and C <= 1024 (alpha/beta and the rows of a frame
 * live in 64 KiB of LDS; one log-prob per thread is prefetched); otherwise ASR_EUNSUPPORTED
 * and the caller runs asr_lattice_fwbw_f32 on the padded matrices.
 */
int asr_lattice_shared_supported(int N, int E, int C);
int64_t asr_lattice_shared_workspace_bytes(int T, int B, int N);
int asr_lattice_shared_fwbw_f32(
    const float *lp, int T, int B, int C, const int32_t *lens, int N, int E,
    const int32_t *in_ptr, const uint32_t *in_arc, const int32_t *out_ptr, const uint32_t *out_arc,
    const float *term, const int32_t *order_in, int n_light_in, int lanes_in,
    const int32_t *order_out, int n_light_out, int lanes_out, float neg_inf, float grad_sign,
    int accumulate, float *out_logZ, float *out_grad, float *out_logZ_bwd, void *workspace,
    int64_t workspace_bytes, void *stream);
int asr_lattice_shared_forward_f32(
    const float *lp, int T, int B, int C, const int32_t *lens, int N, int E,
    const int32_t *in_ptr, const uint32_t *in_arc, const float *term, const int32_t *order_in,
    int n_light_in, int lanes_in, float neg_inf, int viterbi, float *out_score,
    int32_t *out_best_il, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * CTC forced alignment: batched Viterbi with traceback over the reference's dense CTC lattices
 * (csrc/ctc_align.hip).  Replaces, for a whole batch in one launch, mono_CTC_viterbi_align
 * (att_speech/modules/ctc_losses.py:475-481) and bi_CTC_viterbi_align (:505-511), i.e.
 * raw_generic_viterbi (:412-457) with start states {0, 1} and terminal states {N-2, N-1} over the
 * matrices of get_CTC_matrices_mono (:67-94) / get_CTC_matrices_bicontext (:111-166, without
 * loop_using_symbol_repetitions).  The kernel reads no graph matrices: it derives the class of
 * each of the N = 2 L + 1 states and its self-loop / skip flags from the labels.  These entry
 * points are additions: no existing signature changes, so the ABI version stays 24.
 *
 *   lp         [T,B,C] f32   log-probs, time-major; must be finite (the reference itself turns a
 *                            -inf into NaN in its emission product)
 *   lens       [B]     i32   frames of each utterance (any order)
 *   labels     [B,Lmax] i32  transcripts, padded; context_order 2 reduces them modulo S
 *   label_lens [B]     i32
 *   S                        symbols including the blank (context_order 2: S * S <= C)
 *   context_order            1 (mono) or 2 (bicontext with contextual blanks)
 *   allow_nonblank_selfloops, eval_repeats_in_context: the bicontext options (:111-113)
 *   out_cost     [B]   f64   -log-prob of the best alignment; +inf when there is none
 *   out_frames   [B,T] i32   class emitted at each frame (the reference's `sol`)
 *   out_states   [B,T] i32   lattice state at each frame (2 i + 1 = label i, even = blanks)
 *   out_segments [B,Lmax,2] i32  (first frame of label i, one past its last)
 *   workspace: asr_ctc_align_workspace_bytes(T,B,Lmax) bytes (0, and NULL accepted, when the
 *              back-pointers of an utterance, T * ceil4(ceil(N/4)) bytes, fit 48 KiB of LDS)
 *
 * The accumulator is fp64 and each step adds one float32 value, as in the reference; the three
 * candidates are compared in ascending source order with a strict `>` (np.argmax: first
 * maximum), and of the terminal states N-2 wins a tie: cost, path and ties are bit-identical to
 * the reference.  Rows t >= lens[b] and labels i >= label_lens[b] are -1.  An utterance with no
 * alignment (lens[b] too short for the transcript, lens[b] == 0 or > T, label_lens[b] == 0 or
 * > Lmax, a negative label, a mono label >= C) gets cost +inf and -1 everywhere.
 * asr_ctc_align_supported: T >= 1, 1 <= Lmax <= 511, C >= 1 (one wave holds N <= 256, four waves
 * N <= 1023); otherwise asr_ctc_align_f64 returns ASR_EUNSUPPORTED and the caller aligns on the
 * host.  ASR_EINVAL: null pointers, context_order outside {1, 2}, S * S > C, a workspace that is
 * too small.  One workgroup per utterance, no atomics.
 */
int asr_ctc_align_supported(int T, int Lmax, int C);
int64_t asr_ctc_align_workspace_bytes(int T, int B, int Lmax);
int asr_ctc_align_f64(const float *lp, const int32_t *lens, const int32_t *labels,
                      const int32_t *label_lens, int B, int T, int C, int Lmax, int S,
                      int context_order, int allow_nonblank_selfloops, int eval_repeats_in_context,
                      double *out_cost, int32_t *out_frames, int32_t *out_states,
                      int32_t *out_segments, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Beam-pruned Viterbi decoding over one shared WFST (csrc/wfst_decode.hip): the search the
 * reference leaves to Kaldi's decode-faster over CTC_LG_syms.fst (egs/wsj/ctc_kaldi_decode.sh:144-147,
 * --beam, --acoustic-scale, --allow-partial), batched, as frame-synchronous token passing with the
 * order-independent semantics of DESIGN.md section 4.19.  These entry points are additions: no
 * existing signature changes, so the ABI version stays 24.
 *
 *   lp            f32   log-probs: utterance b, frame t, class c at lp[t * frame_stride + b * C + c]
 *                       (a [T,B,C] tensor has frame_stride = B * C; a chunk of the utterances of a
 *                       larger batch keeps that batch's stride).  Frames t >= lens[b] are never read.
 *   lens          [B] i32   frames of each utterance, 1 <= lens[b] <= T (otherwise an empty result)
 *   the graph: tropical, N states, A arcs in CSR by source, start state `start`
 *     arc_ptr     [N+1] u32   arcs of state s are [arc_ptr[s], arc_ptr[s+1]); "arc index" below
 *     arc_src, arc_dst  [A] i32
 *     arc_ilabel  [A] i32     0: non-emitting; i > 0 reads class i - 1 (decoding_utils/ctc_fst.py:42-44)
 *     arc_olabel  [A] i32     0: no output
 *     arc_weight  [A] f32     finite costs of any sign
 *     final_cost  [N] f32     +inf: not final
 *     eps_ptr [N+1] u32, eps_arc [E] u32: the arc indices of the non-emitting arcs, by source
 *     eps_rank    [N] i32     every non-emitting arc goes from a lower to a higher rank (the
 *                             non-emitting sub-graph is acyclic); num_ranks = 1 + the highest rank a
 *                             non-emitting arc leaves, 0 without such arcs
 *   beam >= 0 (+inf: no pruning), acoustic_scale, allow_partial
 *   list_cap, log_cap: tokens one frame may hold / back-pointer records one utterance may write;
 *     word_cap: output labels one path may carry.  An utterance that outgrows any of them gets
 *     out_overflow[b] = 1 and no result: the caller redoes it elsewhere.  No retry on the device.
 *   threads: 0 (512 threads per workgroup above 256 utterances, 1024 up to there: measured,
 *     DESIGN.md section 4.19), or 256 / 512 / 1024 for timing runs
 *   out_cost [B] f32 (+inf: no result), out_reached_final [B] i32, out_alignment [B,T] i32 (the
 *     ilabel of the emitting arc of every frame, -1 beyond lens[b] or without a result),
 *     out_num_active [B,T] i32 (tokens that survive the frame's last prune; the frame lens[b] - 1 is
 *     not pruned), out_words [B,word_cap] i32 with out_num_words [B]: the olabels != 0 along the
 *     path, LAST word first.
 *   workspace: asr_wfst_decode_workspace_bytes(N, B, list_cap, log_cap) bytes = per utterance
 *     12 N + 20 list_cap + 8 log_cap, rounded; the caller splits a batch whose tables exceed its budget.
 *
 * Arithmetic (all fp32, one rounding per operation, no contraction): a = -(acoustic_scale * lp);
 * an emitting arc proposes (c(src) + w) + a[ilabel] to its destination, a non-emitting arc
 * c(src) + w, in rank order; a state's cost is the minimum of its proposals and the smallest arc
 * index wins among equal ones, whether emitting or not; survivors satisfy c <= min c + beam, after
 * the emitting phase and again after the closure; the answer is argmin c + final over the final
 * states reached after the last frame (ties: the smallest state id), else with allow_partial
 * argmin c.  asr_wfst_decode_supported: 1 <= N < 2^31, A < 2^32 - 1, 1 <= C <= 4096, T >= 1;
 * otherwise ASR_EUNSUPPORTED.  ASR_EINVAL: null pointers, start outside the graph, a negative or NaN
 * beam, capacities outside [1, 2^31), threads outside {0, 256, 512, 1024}, a workspace that is too small.  One workgroup per
 * utterance, workgroup barriers only; every loop is bounded by lens, num_ranks, the capacities
 * and the arc counts, and out-of-range indices of a broken graph are skipped.
 */
int asr_wfst_decode_supported(int64_t N, int64_t A, int C, int T);
int64_t asr_wfst_decode_workspace_bytes(int64_t N, int B, int64_t list_cap, int64_t log_cap);
int asr_wfst_decode_f32(const float *lp, int64_t frame_stride, const int32_t *lens, int T, int B, int C,
                        int64_t N, int64_t A, const uint32_t *arc_ptr, const int32_t *arc_src,
                        const int32_t *arc_dst, const int32_t *arc_ilabel, const int32_t *arc_olabel,
                        const float *arc_weight, const float *final_cost, const uint32_t *eps_ptr,
                        const uint32_t *eps_arc, int64_t E, const int32_t *eps_rank, int num_ranks,
                        int start, float beam, float acoustic_scale, int allow_partial, int64_t list_cap,
                        int64_t log_cap, int word_cap, int threads, float *out_cost,
                        int32_t *out_reached_final,
                        int32_t *out_alignment, int32_t *out_num_active, int32_t *out_words,
                        int32_t *out_num_words, int32_t *out_overflow, void *workspace,
                        int64_t workspace_bytes, void *stream);

/*
 * Lattice generation from the same search (csrc/wfst_lattice.hip): where the reference runs
 * decode-faster once per acoustic scale (egs/wsj/ctc_kaldi_decode.sh:160-163), one search keeps
 * every arc within lattice_beam of the best path, graph cost and acoustic score apart
 * (latgen-faster), with the order-independent semantics of DESIGN.md section 4.20.  Additions
 * again: the ABI version stays 24.
 *
 * lp, lens, the graph, beam, acoustic_scale, allow_partial, list_cap, log_cap, threads: as for
 * asr_wfst_decode_f32 (arc_olabel is not read).  The forward IS that search: out_cost and
 * out_reached_final are the same bits.
 *   lattice_beam >= 0 (+inf: every arc with a finite value)
 *   node_cap, arc_cap: nodes / arcs one utterance may keep
 *   out_overflow [B] i32: 0, or which capacity the utterance outgrew (1 a token list, 2 the log,
 *     3 node_cap, 4 arc_cap); it then has no result and the caller redoes it elsewhere
 *   out_num_nodes, out_num_arcs [B] i32 (0 nodes: no lattice, out_cost = +inf)
 *   node_time, node_state [B,node_cap] i32, node_alpha, node_beta [B,node_cap] f32
 *   lat_src, lat_dst [B,arc_cap] i32 (node indices of the utterance), lat_arc [B,arc_cap] u32
 *     (arc index in the graph), lat_lp [B,arc_cap] f32 (the class score read, unscaled; 0 for
 *     non-emitting arcs).  Nodes and arcs come in no particular order: the caller sorts.
 *   workspace: asr_wfst_lattice_workspace_bytes(N, B, T, list_cap, log_cap) bytes = per utterance
 *     12 N + 20 list_cap + 24 log_cap + 8 (T + 2), rounded.
 *
 * Time k = frames consumed.  A node is a token (k, state) that exists after the closure at time k,
 * alpha its cost.  Lattice arcs: emitting arcs from the survivors of time k - 1 whose proposal
 * (alpha + w) + a[ilabel] is finite and within the threshold of frame k's first prune;
 * non-emitting arcs between tokens of one time with alpha + w finite.  beta: final cost at time
 * lens[b] (0 everywhere when no final state was reached and allow_partial is set), and backwards
 * beta(u) = min over the lattice arcs u -> v of x + beta(v), x = w + a[ilabel] (w for non-emitting
 * arcs), through a 32-bit atomic minimum over the order-preserving key.  Kept: the arcs with
 * alpha(u) + (x + beta(v)) finite and <= out_cost + lattice_beam, and the arcs of the search's own
 * traceback; the nodes are their end points and the start token.  All fp32, one rounding per
 * operation.  One workgroup per utterance does forward and backward in one launch, workgroup
 * barriers only; every loop is bounded by lens, num_ranks, the capacities and the arc counts.
 */
int asr_wfst_lattice_supported(int64_t N, int64_t A, int C, int T);
int64_t asr_wfst_lattice_workspace_bytes(int64_t N, int B, int T, int64_t list_cap, int64_t log_cap);
int asr_wfst_lattice_f32(const float *lp, int64_t frame_stride, const int32_t *lens, int T, int B, int C,
                         int64_t N, int64_t A, const uint32_t *arc_ptr, const int32_t *arc_src,
                         const int32_t *arc_dst, const int32_t *arc_ilabel, const int32_t *arc_olabel,
                         const float *arc_weight, const float *final_cost, const uint32_t *eps_ptr,
                         const uint32_t *eps_arc, int64_t E, const int32_t *eps_rank, int num_ranks,
                         int start, float beam, float lattice_beam, float acoustic_scale,
                         int allow_partial, int64_t list_cap, int64_t log_cap, int64_t node_cap,
                         int64_t arc_cap, int threads, float *out_cost, int32_t *out_reached_final,
                         int32_t *out_num_nodes, int32_t *out_num_arcs, int32_t *node_time,
                         int32_t *node_state, float *node_alpha, float *node_beta,
                         int32_t *lat_src, int32_t *lat_dst, uint32_t *lat_arc, float *lat_lp,
                         int32_t *out_overflow, void *workspace, int64_t workspace_bytes,
                         void *stream);

/*
 * Dynamic programmes over a batch of such lattices that stays on the device (csrc/lattice_dp.hip,
 * DESIGN.md section 4.21): re-ranking under any number of (acoustic scale, LM scale) pairs in one
 * launch (lattice-best-path per scale), and arc / node posteriors by a log-semiring
 * forward-backward (lattice-to-post).  Additions again: the ABI version stays 24.
 *
 * The batch: B lattices laid end to end, N nodes, A arcs, in the canonical form (nodes by
 * (utterance, time, state), arcs by (utterance, source node, graph arc index)).
 *   node_off, arc_off, level_off [B+1] i64, on the device, and h_* the same words on the host: from
 *     0 to N / A / L, never decreasing (checked on the host copies before anything is launched)
 *   node_time, node_state [N] i32; node_level [N] i32 the node's level, an index into level_ptr:
 *     levels ascend by (utterance, time, epsilon rank of the state) and every arc rises in level
 *   lat_src, lat_dst [A] i32 node indices within the utterance, lat_arc [A] i64 arc index in the
 *     graph, lat_lp [A] f32 the unscaled class score (0 on non-emitting arcs)
 *   level_ptr [L+1] i32, level_node [N] i32: the nodes (batch indices) of level l are
 *     level_node[level_ptr[l] .. level_ptr[l+1]); utterance b owns the levels level_off[b] ..
 *   in_ptr [N+1] i32, in_arc [A] i32: the in-arcs (batch indices) of node v, in the stored order
 *   out_ptr [N+1] i32: the out-arcs of node v are the arcs out_ptr[v] .. out_ptr[v+1]
 *   num_frames, reached_final [B] i32; own_scale [B] f64 the acoustic scale of each search
 *   the graph: arc_weight [G] f32, arc_olabel [G] i32, final_cost [num_states] f32, start
 *   b_begin, b_count: the utterances this launch serves (the workspace covers their nodes only)
 *   threads: 0 (= 64), 64, 128 or 256 lanes per workgroup
 *
 * Arc cost x = fl(fl(lm w) - fl(sc lp)) in fp64, no contraction; end(v) = final(state) at time
 * num_frames when reached_final, 0 at that time otherwise, +inf elsewhere.
 *
 * asr_lattice_bestpath_f64: per pair p (acoustic_scales[p] NaN: own_scale) and utterance
 *   cost(start) = 0, cost(v) = min over in-arcs of cost(u) + x; back-pointer: of the in-arcs that
 *   attain it and are finite, the smallest graph arc index; winner: the smallest node index among the
 *   minima of cost(v) + fl(lm end(v)); traceback from there, graph cost = end + sum of w, acoustic
 *   cost = - sum of lp, added in that order.  IEEE semantics as numpy: a NaN among the utterance's
 *   costs means no path.  No path: (+inf, +inf, +inf) and 0 words.
 *   out_cost [P,B,3] f64 (cost, graph cost, acoustic cost), out_num_words [P,B] i32, out_words [P,L]
 *   i32 (utterance b's words of pair p start at p L + level_off[b]; a path has at most one arc per
 *   level), out_status [P,B] i32: 1 when an index read from the arrays was out of range or a level
 *   did not rise (the utterance then has no result).
 *   workspace: asr_lattice_bestpath_workspace_bytes(nodes of the launch, P) = 12 bytes per node and
 *   pair, rounded.  One workgroup per (pair, utterance), workgroup barriers only.
 *
 * asr_lattice_posterior_f64: fwd(start) = 0, fwd(v) = logsumexp over in-arcs of fwd(u) - x; bwd(v) =
 *   logsumexp of -fl(lm end(v)) (end nodes) and bwd(d) - x over out-arcs; each by one lane in the
 *   stored order, max then sum: no atomics on results, run-to-run identical bits.
 *   out_log_z [B] = bwd(start) (-inf: no lattice), out_arc_log_post [A] = fwd(src) - x + bwd(dst) -
 *   log_z, out_node_log_post [N] = fwd + bwd - log_z (-inf where a term is), out_status [B] as above.
 *   workspace: asr_lattice_posterior_workspace_bytes(nodes of the launch) = 16 bytes per node, rounded.
 */
int asr_lattice_bestpath_supported(int64_t N, int64_t A, int64_t L);
int64_t asr_lattice_bestpath_workspace_bytes(int64_t num_nodes, int num_pairs);
int asr_lattice_bestpath_f64(
    int B, int b_begin, int b_count, int num_pairs, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    const double *acoustic_scales, const double *lm_scales, int64_t num_states, int64_t num_graph_arcs,
    const float *arc_weight, const int32_t *arc_olabel, const float *final_cost, int start, int threads,
    double *out_cost, int32_t *out_num_words, int32_t *out_words, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream);
int asr_lattice_posterior_supported(int64_t N, int64_t A, int64_t L);
int64_t asr_lattice_posterior_workspace_bytes(int64_t num_nodes);
int asr_lattice_posterior_f64(
    int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, double *out_log_z,
    double *out_arc_log_post, double *out_node_log_post, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream);

/*
 * asr_lattice_nbest_f64: the n cheapest DISTINCT word sequences of every lattice of such a batch, in
 * one launch (csrc/lattice_dp.hip; LatticeBatch.nbest of
 * att_speech/wfst_lattice.py is its numpy twin and gives the same bits).  Additions: the ABI version
 * stays 24.  The batch, b_begin / b_count and x as above; threads: 64, 128 or 256 lanes per workgroup,
 * 0 = 256 (a wave per node: four nodes of a level at a time); acoustic_scale NaN: own_scale.
 *
 * A k-best dynamic programme backwards over the levels.  Every node v keeps a list of at most n
 * entries (c, len, h, arc, rank): the cost of a word suffix from v to an end, its number of words, a
 * 64-bit hash of it, the out-arc taken (-1: stop at v), the index into the list of that arc's
 * destination.  e(v) = fl(lm final(state)) at time num_frames when reached_final, 0 at that time
 * otherwise, +inf elsewhere.  The candidates of v:
 *   the stop entry (e(v), 0, 0, -1, 0) when e(v) < +inf;
 *   for every out-arc j and every entry r of list(dst_j): c' = fl(x_j + c_r), dropped unless
 *   c' < +inf (which drops NaN too), len' = len_r + (olabel_j != 0), h' = olabel_j != 0 ?
 *   h_r * 0x9E3779B97F4A7C15 + olabel_j + 1 (mod 2^64) : h_r.
 * They are ordered by (c', len', h', arc, rank) ascending; of candidates with equal (len', h') only
 * the first survives; list(v) is the first n survivors.  Two suffixes are the same sequence iff
 * (len, h) agree: a 64-bit hash identity, and a collision would drop one of two sequences from a
 * list, nothing else.  The result is this order's, whatever the schedule: no atomics on results.
 * Read-out: the entries of the start node (time 0, state `start`) are followed forwards along (arc,
 * rank); the non-zero output labels are the words, and the cost is summed forwards, g = 0,
 * g = fl(g + x_j) per arc, then fl(g + e(end)), as LatticeBatch.best_paths sums it.
 *   out_count [B] i32 entries of utterance b (0: no nodes, no start node or no finite path);
 *   out_cost [B, n] f64, out_num_words [B, n] i32, in the list's order (the caller sorts by (cost,
 *   words)); out_words [n L] i32: the words of entry i of utterance b start at n level_off[b] +
 *   i levels(b) (a path has at most one arc per level); out_status [B] i32 as above, also raised by
 *   a rank outside the destination's list or an entry whose destination does not sit higher.
 *   n: 1 .. ASR_LATTICE_NBEST_MAX (more: ASR_EUNSUPPORTED; less: ASR_EINVAL).
 *   workspace: asr_lattice_nbest_workspace_bytes(nodes of the launch, n) = n entries of 28 bytes (cost
 *   f64, hash u64, len, arc, rank i32) and one i32 count per node, rounded.  The outputs are not part
 *   of it.  One workgroup per utterance, one wave per node of a level, workgroup barriers only.
 */
#define ASR_LATTICE_NBEST_MAX 64
int asr_lattice_nbest_supported(int64_t N, int64_t A, int64_t L, int n);
int64_t asr_lattice_nbest_workspace_bytes(int64_t num_nodes, int n);
int asr_lattice_nbest_f64(
    int B, int b_begin, int b_count, int n, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, int32_t *out_count,
    double *out_cost, int32_t *out_num_words, int32_t *out_words, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream);

/*
 * asr_lattice_mbr_f64: minimum-Bayes-risk decoding of every lattice of such a batch in one launch
 * (csrc/lattice_dp.hip; Xu, Povey, Mangu, Zhu 2011, Kaldi's lattice-mbr-decode;
 * LatticeBatch.mbr of att_speech/wfst_lattice.py is its numpy twin and gives the same results with ==).
 * Additions: the ABI version stays 24.  The batch, b_begin / b_count, x and end(v) as above; threads: 64,
 * 128 or 256 lanes per workgroup, 0 = 256; acoustic_scale NaN: own_scale.
 *
 * Lattice model, per utterance.  A virtual end node E; every node v with end(v) < inf has a stop arc
 * v -> E without a word; an arc's word is the olabel of its graph arc, 0 = no word.  The start node is
 * the node (time 0, state `start`); arcs into it are ignored.
 * Conditional posteriors: pi_j = exp((fwd(src_j) - x_j) - fwd(dst_j)), pi_stop(v) = exp((fwd(v) -
 *   fl(lm end(v))) - log_z), fwd the forward score of asr_lattice_posterior_f64 and log_z the log-sum of
 *   the stop terms (one lane, node order, max then sum); 0 where a term is infinite or the value is not
 *   > 0.  arc_cond [A] / end_cond [N] f64 give them; NULL (either): computed here as phase 0.
 * Hypothesis w_1..w_Q in slot form r_1..r_S, S = 2Q + 1: r_q = 0 at odd q (gaps), r_2k = w_k.
 * Losses, delta = 1e-5: sub(w, r) = 0 if w == r else 1 + delta; ins(w) = 0 if w == 0 else 1 + delta;
 *   del(r) = 0 if r == 0 else 1.
 * Forward: alpha'(s, 0) = 0, alpha'(s, q) = alpha'(s, q-1) + del(r_q) at the start node s; for every
 *   other node v (E last) and every in-arc (u -> v, w, pi) with pi > 0:
 *     a(0) = alpha'(u, 0) + ins(w),
 *     a(q) = min(A1 = alpha'(u, q-1) + sub(w, r_q), A2 = alpha'(u, q) + ins(w), A3 = a(q-1) + del(r_q)),
 *     alpha'(v, q) = sum over the in-arcs of pi a(q);   risk = alpha'(E, S).
 * Backward: beta'(E, S) = 1; nodes by descending level (E first); per in-arc, q = S .. 1:
 *     b(q) += pi beta'(v, q); case 1 (A1 <= A2 and A1 <= A3): beta'(u, q-1) += b(q), gamma(q, w) += b(q),
 *     tau(q, w) += b(q) time(v); case 2 (else A2 <= A3): beta'(u, q) += b(q); case 3: b(q-1) += b(q),
 *     gamma(q, 0) += b(q); finally b(0) += pi beta'(v, 0), beta'(u, 0) += b(0).  At the start node case 3
 *     alone is applied to beta'(s, .).  For every slot the gamma(q, .) sum to 1.
 * Update: r_q <- argmax_w gamma(q, w); among equal maxima the current r_q if it is one, else the smallest
 *   label; zeros dropped, gaps re-inserted.
 * Iteration: start from init_words (utterance b: init_num_words[b] words at init_words + b max_words) or,
 *   both NULL, from the tropical best path under the tie rule of asr_lattice_bestpath_f64; evaluate,
 *   update; stop when the words did not change or after max(1, max_iterations) evaluations
 *   (max_iterations = 0 scores the given sentences unchanged).  The result is the last EVALUATED
 *   hypothesis's: confidence of word k = gamma(2k, w_k), frame = tau / gamma to the nearest integer.
 * Arithmetic (the order of additions cannot matter): alpha' and a are int64 at 2^-40 (1 = 2^40, delta =
 *   10995116); beta', b, gamma int64 at 2^-52; every product is llrint(pi (double)v), round-half-even,
 *   uncontracted; tau adds (b >> 12) time(v) and frame = rint((double)tau / (double)(gamma >> 12)) (0 when
 *   gamma >> 12 is 0); minima, cases and the argmax are integer comparisons, entries with b = 0 are
 *   skipped.  The rounding error of the risk is at most (levels x in-degree) 2^-41.
 *   max_words: 1 .. ASR_LATTICE_MBR_MAX_WORDS, the words a hypothesis may hold in this launch.
 *   out_num_words [B] i32; out_words, out_frames [B, max_words] i32, out_confidence [B, max_words] f64
 *   (utterance b's at b max_words); out_risk [B] f64 (+inf and 0 words, 0 iterations: no nodes, no start
 *   node, no complete path, or a NaN among the best path's costs); out_iterations [B] i32;
 *   out_status [B] i32 bits: 1 an index out of range or a level that does not rise, 2 the sausage
 *   buffer overflowed, 4 the hypothesis (given, the best path's, or after an update) holds more than
 *   max_words words; with 2 or 4 the caller redoes the utterance on the host.
 *   The sausage: out_sausage_key, _gamma, _tau [B, sausage_cap] i64, an open-addressing table the kernel
 *   accumulates in: key = slot << 32 | word (-1: empty), gamma at 2^-52, tau as above; the entries of the
 *   last evaluation with key >= 0 and gamma > 0 are the confusion network, out_sausage_count [B] their
 *   number, in no particular order.
 *   workspace: asr_lattice_mbr_workspace_bytes(nodes of the launch, max_words) = 16 (2 max_words + 2) + 8
 *   bytes per node, rounded (alpha', beta', fwd; a is recomputed in the backward pass, so there is no
 *   per-arc chain).  One workgroup per utterance and one launch for all iterations; a wave owns a node
 *   of a level and takes its in-arcs in turn, its lanes run over the slots; A3 is a min-plus prefix scan
 *   over the lanes and b a segmented suffix sum, both exact in integers, with a carry between 64-slot
 *   rounds; beta', gamma and tau are summed with 64-bit integer atomics; workgroup barriers only.
 */
#define ASR_LATTICE_MBR_MAX_WORDS 255
int asr_lattice_mbr_supported(int64_t N, int64_t A, int64_t L, int max_words);
int64_t asr_lattice_mbr_workspace_bytes(int64_t num_nodes, int max_words);
int asr_lattice_mbr_f64(
    int B, int b_begin, int b_count, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *h_level_off, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *node_time, const int32_t *node_state, const int32_t *node_level,
    const int32_t *lat_src, const int32_t *lat_dst, const int64_t *lat_arc, const float *lat_lp,
    const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr, const int32_t *in_arc,
    const int32_t *out_ptr, const int32_t *num_frames, const int32_t *reached_final, const double *own_scale,
    double acoustic_scale, double lm_scale, int64_t num_states, int64_t num_graph_arcs, const float *arc_weight,
    const int32_t *arc_olabel, const float *final_cost, int start, int threads, const double *arc_cond,
    const double *end_cond, const int32_t *init_words, const int32_t *init_num_words, int max_iterations,
    int max_words, int64_t sausage_cap, int32_t *out_num_words, int32_t *out_words, double *out_confidence,
    int32_t *out_frames, double *out_risk, int32_t *out_iterations, int32_t *out_status,
    int32_t *out_sausage_count, int64_t *out_sausage_key, int64_t *out_sausage_gamma, int64_t *out_sausage_tau,
    void *workspace, int64_t workspace_bytes, void *stream);

/*
 * asr_lattice_oracle_i32: the lattice oracle of every lattice of such a batch in one launch (csrc/
 * lattice_oracle.hip; Kaldi's lattice-oracle; LatticeBatch.oracle of
 * att_speech/wfst_lattice.py is its numpy twin and gives the same results with ==): the complete path whose
 * words are nearest to a reference in word edit distance.  Additions: the ABI version stays 24.  The batch,
 * b_begin / b_count, x and end(v) as above; threads: 64, 128 or 256 lanes per workgroup, 0 = 256;
 * acoustic_scale NaN: own_scale.
 *
 * Lattice model, per utterance, as for asr_lattice_mbr_f64: the start node s is the node (time 0, state
 * `start`), arcs into it are ignored; v is an end node when end(v) < inf; an arc's word w is the olabel of its
 * graph arc, 0 = no word.  The reference r_1..r_R: ref_num_words[b] = R labels > 0 at ref_words + b max_words
 * (labels the graph does not have can only be substituted or deleted).
 * Arithmetic: int32; U = 2^30 stands for unreachable and every sum is clamped with min(., U); supported only
 *   if levels + max_words < U (asr_lattice_oracle_supported).
 * Forward: D(s, q) = q for q = 0..R.  Every other node v in level order, per in-arc j = (u -> v, w) in the
 *   stored in_arc order: w == 0: c_j(q) = D(u, q); else c_j(0) = D(u, 0) + 1 and for q >= 1
 *   c_j(q) = min(D(u, q-1) + (w != r_q), D(u, q) + 1).  D0(v, q) = min_j c_j(q) (U without in-arcs);
 *   D(v, q) = min(D0(v, q), D(v, q-1) + 1) = q + min_{i <= q} (D0(v, i) - i).
 * Result: errors = min over the end nodes of D(v, R), v* the smallest node among the minima (the tie rule of
 *   asr_lattice_bestpath_f64); no result (out_errors = -1, counts and words 0, cost +inf) without nodes, start
 *   node or end node, or when the minimum is >= U.
 * Traceback from (v*, R).  At (v, q), v != s: the first in-arc in the stored order with c_j(q) == D(v, q);
 *   if w != 0, q >= 1 and D(u, q-1) + (w != r_q) == D(v, q): a diagonal step (correct when w == r_q, else a
 *   substitution), ref_frames[q-1] = time(v), on to (u, q-1); else if w != 0: an insertion, on to (u, q);
 *   else on to (u, q).  If no in-arc attains D(v, q): a deletion, ref_frames[q-1] = -1, on to (v, q-1).  At s
 *   the remaining q positions are deletions.  errors = sub + ins + del and cor + sub + del = R.  Ties among
 *   paths of the least distance are broken by this rule, not by cost.
 *   ref_words [B, max_words] i32, ref_num_words [B] i32 (outside 0 .. max_words: status bit 1); max_words:
 *   1 .. ASR_LATTICE_ORACLE_MAX_WORDS.  out_errors [B] i32; out_counts [B, 4] i32: substitutions, insertions,
 *   deletions, correct; out_num_words [B] and out_words [L] i32: the non-zero olabels of the path in forward
 *   order, utterance b's at level_off[b] (the kernel keeps the path's arcs there meanwhile);
 *   out_ref_frames [B, max_words] i32; out_cost [B] f64: the path's cost summed forwards as the read-out of
 *   asr_lattice_nbest_f64 sums it, g = 0, g = fl(g + x_j) per arc, then fl(g + fl(lm end(v*)));
 *   out_status [B] i32 bit 1: an index out of range or a level that does not rise.
 *   workspace: asr_lattice_oracle_workspace_bytes(nodes of the launch, max_words) = 4 (max_words + 1) bytes
 *   per node, rounded: the rows D(v, .), kept for the traceback.  One workgroup per utterance; a wave owns a
 *   node of a level and takes its in-arcs in turn, its lanes run over q in rounds of 64; the chain is a prefix
 *   minimum over the lanes with a carry between the rounds; the traceback is one wave's, a lane per in-arc, the
 *   first hit by ballot; workgroup barriers only, no atomics on global memory: two runs give the same words.
 */
#define ASR_LATTICE_ORACLE_MAX_WORDS 1023
int asr_lattice_oracle_supported(int64_t N, int64_t A, int64_t L, int max_words);
int64_t asr_lattice_oracle_workspace_bytes(int64_t num_nodes, int max_words);
int asr_lattice_oracle_i32(
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
    int64_t workspace_bytes, void *stream);

/*
 * asr_lattice_lmrescore_*: lattice o back-off n-gram LM for a batch that stays on the device
 * (csrc/lattice_lm.hip; att_speech/lattice_lm.py states the semantics and holds the
 * numpy twin, which gives the same bits).  Three entries, called in this order for the utterances
 * [b_begin, b_begin + b_count) of a batch in the layout of asr_lattice_bestpath_f64; src_global / dst_global
 * [A] int64 are the arcs' end points as batch node indices, arc_utt [A] int64 their utterance.
 *
 * The LM in back-off form: lm_ptr [lm_states + 1], lm_label / lm_dst / lm_weight [lm_arcs] the non-epsilon
 * arcs by (state, label), labels distinct within a state; lm_bo_dst [lm_states] (-1: none) and lm_bo_w the
 * back-off arc; label_map [label_map_len] int64 takes an output label of the graph to a label of the LM
 * (<= 0 or outside the map: out of vocabulary, the arc costs oov_cost and keeps the LM state; +inf drops it).
 *
 *   expand   per node the sorted distinct LM states that reach it, at most max_lm_states
 *            (1 .. ASR_LATTICE_LMRESCORE_MAX_STATES) in the workspace; out_count [N] their number,
 *            out_status [B]: bit 0 an utterance outgrew max_lm_states (its counts are then meaningless and
 *            the caller zeroes them), bit 1 inconsistent index arrays.
 *   emit     node_slot [nodes of the launch + 1] and arc_slot [arcs of the launch + 1] are the exclusive prefix
 *            sums of count over the nodes and of count[source] over the arcs; E and M their totals.  Writes the LM
 *            state of every expanded node and, per (arc, LM state of its source), the expanded end points
 *            (launch-local), the source's LM state, the LM cost c (fp64, summed along the back-off chain in
 *            order), weight = fl32(fl64(w) + scale * c), acoustic = -(fl32(own_scale) * lp), and out_ok: 1 kept,
 *            0 dropped as out of vocabulary, -1 inconsistent.  Reads the workspace expand left.
 *   sweep    over an expanded lattice in canonical order with its own level structure (all B utterances in one
 *            launch): alpha, beta in fp32 with one rounding per operation, out_best [B] = min over the end
 *            nodes of (alpha + end) + 0, and out_keep [M] (zero on entry): 1 where alpha(u) + (((w + a) +
 *            beta(v)) + 0) is finite and <= best + lattice_beam (+inf: finite), or the arc lies on the forward
 *            traceback from the first best end node.  No atomics: two runs give the same bits.
 */
#define ASR_LATTICE_LMRESCORE_MAX_STATES 1024
int asr_lattice_lmrescore_supported(int64_t N, int64_t A, int64_t L, int max_lm_states);
int64_t asr_lattice_lmrescore_workspace_bytes(int64_t num_nodes, int max_lm_states);
int asr_lattice_lmrescore_expand(
    int B, int b_begin, int b_count, int max_lm_states, int64_t N, int64_t A, int64_t L, const int64_t *h_node_off,
    const int64_t *node_off, const int64_t *level_off, const int32_t *node_time, const int32_t *node_state,
    const int64_t *src_global, const int64_t *lat_arc, const int32_t *level_ptr, const int32_t *level_node,
    const int32_t *in_ptr, const int32_t *in_arc, int64_t num_graph_arcs, const int32_t *arc_olabel, int start,
    int64_t lm_states, int64_t lm_arcs, const int32_t *lm_ptr, const int32_t *lm_label, const int32_t *lm_dst,
    const double *lm_weight, const int32_t *lm_bo_dst, const double *lm_bo_w, int lm_start, const int64_t *label_map,
    int64_t label_map_len, double oov_cost, int32_t *out_count, int32_t *out_status, void *workspace,
    int64_t workspace_bytes, void *stream);
int asr_lattice_lmrescore_emit(
    int B, int b_begin, int b_count, int max_lm_states, int64_t N, int64_t A, const int64_t *h_node_off,
    const int64_t *h_arc_off, const int64_t *src_global, const int64_t *dst_global, const int64_t *arc_utt,
    const int64_t *lat_arc, const float *lat_lp, const double *own_scale, int64_t num_graph_arcs,
    const int32_t *arc_olabel, const float *arc_weight, int64_t lm_states, int64_t lm_arcs, const int32_t *lm_ptr,
    const int32_t *lm_label, const int32_t *lm_dst, const double *lm_weight, const int32_t *lm_bo_dst,
    const double *lm_bo_w, int lm_start, const int64_t *label_map, int64_t label_map_len, double oov_cost,
    double scale, const int32_t *count, const int64_t *node_slot, const int64_t *arc_slot, int64_t E, int64_t M,
    int32_t *out_lm_state, int32_t *out_src, int32_t *out_dst, int32_t *out_src_lm_state, double *out_lm_cost,
    float *out_weight, float *out_acoustic, int32_t *out_ok, const void *workspace, int64_t workspace_bytes,
    void *stream);
int asr_lattice_lmrescore_sweep(
    int B, int64_t E, int64_t M, int64_t EL, int64_t N, const int64_t *node_off, const int64_t *arc_off,
    const int64_t *level_off, const int32_t *level_ptr, const int32_t *level_node, const int32_t *in_ptr,
    const int32_t *in_arc, const int32_t *out_ptr, const int32_t *src, const int32_t *dst, const float *weight,
    const float *acoustic, const int32_t *lat_node, const int32_t *lm_state, const int32_t *node_time,
    const int32_t *node_state, const int32_t *num_frames, const int32_t *reached_final, int64_t num_states,
    const float *final_cost, int start, int64_t lm_states, const double *lm_final_star, int lm_start, double scale,
    double lattice_beam, int threads, float *out_alpha, float *out_beta, int32_t *out_keep, float *out_best,
    int32_t *out_status, void *stream);

/*
 * asr_lattice_seqtrain_f64: sequence-discriminative training statistics of every lattice of such a batch in
 * one launch (csrc/lattice_train.hip): the denominator of lattice MMI / boosted MMI
 * and the sMBR objective, from the LIVE log_probs.  LatticeBatch.seq_objective of att_speech/wfst_lattice.py is
 * the numpy twin.  Additions: the ABI version stays 24.  The batch, b_begin / b_count and end(v) as for
 * asr_lattice_posterior_f64; threads: 0 (= 64), 64, 128 or 256; acoustic_scale NaN: own_scale.  lat_lp and
 * arc_olabel are part of the common batch arguments and are not read.
 *
 *   arc_ilabel [G] i32: the graph's input labels (class + 1; 0: epsilon); log_probs [T, B, C] f32;
 *   ref [B, T] i32 the reference class of every frame (-1: none), or null: every accuracy 0;
 *   criterion 0 (mmi) or 1 (smbr); boost >= 0, finite.
 * Live score: an emitting arc a (il = arc_ilabel[lat_arc[a]] > 0) into time k = node_time[dst] has
 *   s(a) = (double) log_probs[k-1, b, il-1], acc(a) = (ref[b, k-1] == il-1); an epsilon arc s = 0, acc = 0.
 *   x(a) = fl(fl(fl(lm w) - fl(sc s)) + fl(boost acc)) in fp64, no contraction.
 * fwd, bwd, log_z and gamma(a) = exp(fwd(src) - x + bwd(dst) - log_z) as in asr_lattice_posterior_f64 (max then
 *   sum per node, one owner lane, stored order).  Expected accuracies in linear fp64 over the finite terms:
 *   facc(v) = sum over in-arcs of exp(fwd(u) - x - fwd(v)) (facc(u) + acc(a)), facc(start) = 0;
 *   bacc(u) = sum over out-arcs of exp(bwd(d) - x - bwd(u)) (bacc(d) + acc(a)), the stop term adds 0
 *   (both computed as the weighted sum over exp(term - max) divided by the node's sum);
 *   c_avg = bacc(start), c(a) = facc(src) + acc(a) + bacc(dst).
 * mmi:  out_objective [B] = log_z, out_arc_grad [A] = gamma(a).
 * smbr: out_objective [B] = c_avg, out_arc_grad [A] = gamma(a) (c(a) - c_avg).
 *   No complete path (no nodes, log_z = -inf): objective -inf (mmi) / 0 (smbr), arc_grad 0.
 * The emission index (built once per batch and [T, B, C]): em_arc [num_emitting] i32 the emitting arcs (batch
 *   indices) sorted by (utterance, frame, class, arc); em_ptr [num_segments + 1] i32 the segments of equal
 *   (utterance, frame, class); em_key [num_segments] i64 their offsets ((k-1) B + b) C + il-1 into out_occ,
 *   ascending within an utterance; em_off [B + 1] i64 the segments of every utterance.
 * out_occ [T, B, C] f32, zero on entry: entry em_key[s] = the float rounding of the fp64 sum of out_arc_grad
 *   over segment s in ascending arc order, by one lane; other entries are not written.
 *   d objective[b] / d log_probs[t, b, c] = sc out_occ[t, b, c].
 * out_status [B] i32: 1 when an index read from the arrays was out of range, a level did not rise, an emitting
 *   arc reads a frame or class outside [T, B, C], or the emission index does not list the utterance's emitting
 *   arcs exactly once under their own keys (the utterance then has no result).  Nothing is read or written
 *   out of bounds.
 *   workspace: asr_lattice_seqtrain_workspace_bytes(nodes of the launch) = 32 bytes per node, rounded (fwd, bwd,
 *   facc, bacc).  One workgroup per utterance, workgroup barriers only, no atomics on results: two runs, and
 *   every workgroup size, give the same bits.
 */
int asr_lattice_seqtrain_supported(int64_t N, int64_t A, int64_t L);
int64_t asr_lattice_seqtrain_workspace_bytes(int64_t num_nodes);
int asr_lattice_seqtrain_f64(
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
    void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Feature front-end: Kaldi filter-bank features, deltas and CMVN from padded waveforms in one launch, the
 * arithmetic of the recipes' `compute-fbank-feats --use-energy=true --num-mel-bins=80 | add-deltas` and
 * `apply-cmvn` (egs/wsj/compute_features.sh:17-18), which the reference runs in a Kaldi pipe per DataLoader
 * worker (att_speech/data/kaldi_dataset.py:194-202).  These entry points are additions: the ABI version stays 24.
 *
 * waves: B rows of samples, int16 (waves_int16 = 1) or fp32 (0), row b at waves + b * wave_stride elements, n_max
 *   readable samples per row (wave_stride >= n_max); wave_lens [B] i32 (device) the samples of every utterance
 *   (values beyond n_max are read as n_max).  Samples are taken as they are, with no scaling.
 * Utterance b has T_b = 1 + (N_b - frame_length) / frame_shift frames (0 when N_b < frame_length), at most T_max.
 *   Frame t, x[i] = wave[t frame_shift + i], i < frame_length:
 *     x[i] += dither * z[((b T_max + t) 512 + i)] when dither != 0: the draw of asr_gaussian_noise_f32 under
 *       tag 2 with this seed and iteration (B T_max 512 < 2^34, else ASR_EUNSUPPORTED);
 *     x -= mean(x);  e = log(max(sum x^2, FLT_EPSILON));
 *     x[i] -= preemph x[i-1] for i = frame_length-1 .. 1, x[0] -= preemph x[0];  x[i] *= window[i];
 *     zero-pad to 512, real FFT, P_k = |X_k|^2 for k = 0 .. 255;
 *     m_j = sum over k in [first_j, end_j) of mel_w[off_j + k - first_j] P_k;  log(max(m_j, FLT_EPSILON)).
 *   The F = num_mel_bins + use_energy static features are [e, m_0 ..] (energy first) or [m_0 ..].
 * Tables (device, fp32, built by the host in fp64 and rounded once): window [frame_length]; twiddles [512, 2] =
 *   (cos, -sin)(2 pi j / 512); mel_idx [num_mel_bins, 3] i32 = (first, end, off) with 0 <= first <= end <= 256;
 *   mel_w [mel_w_len], 1 <= mel_w_len <= 512: an FFT bin feeds at most two banks (a bank whose range leaves
 *   the table counts as empty).
 * Channels C = delta_order + 1: channel c of frame t = sum_j s_c[j] static[clamp(t + j, 0, T_b - 1)] with
 *   s_1 = [-2 .. 2] / 10 and s_2 = s_1 * s_1 (9 taps); the clamp repeats the utterance's own edge frames.
 * CMVN: cmvn_offset, cmvn_scale [F C] in the column order [static | delta | delta-delta] (entry c F + f), either
 *   may be NULL: y = (x - offset) scale.
 * out [B, T_max, F, C] f32, every entry written: exactly 0 at t >= T_b.  feat_lens [B] i32 (device) = T_b.
 * fp32 with every sum in a fixed order: two runs give the same bits, and without dither an utterance's rows do not
 *   depend on B, its position in the batch or T_max.
 * asr_fbank_supported: padded == 512, 256 < frame_length <= 512, frame_shift >= 1, 1 <= num_mel_bins <= 128,
 *   0 <= delta_order <= 2, delta_window == 2; otherwise asr_fbank_f32 returns ASR_EUNSUPPORTED.  ASR_EINVAL,
 *   before anything is launched: null pointers, negative sizes, mel_w_len outside 1 .. 512, wave_stride < n_max, T_max < 1 with B > 0,
 *   non-positive frame_length, frame_shift or num_mel_bins, a negative delta_order, flags outside {0, 1}.
 */
int asr_fbank_supported(int frame_length, int frame_shift, int padded, int num_mel_bins, int delta_order,
                        int delta_window);
int asr_fbank_f32(const void *waves, int64_t wave_stride, int n_max, int waves_int16, const int32_t *wave_lens,
                  int B, int T_max, const float *window, const float *twiddles, const int32_t *mel_idx,
                  const float *mel_w, int mel_w_len, int frame_length, int frame_shift, int padded,
                  int num_mel_bins, int use_energy, int delta_order, int delta_window, float preemph,
                  const float *cmvn_offset, const float *cmvn_scale, float dither, uint64_t seed,
                  uint64_t iteration, float *out, int32_t *feat_lens, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASR_AMD_H */
