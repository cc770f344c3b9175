/*
 * capmi.h -- C ABI of libcapmi.so, the MI355X (gfx950 / CDNA4) caption-decoding backend.
 *
 * The reference (ruotianluo/ImageCaptioning.pytorch) has NO native/FFI boundary: its hot path is
 * Python calling torch.nn ops.  This header is therefore the boundary a
 * maintainer would bind with ctypes from the reference's own Python classes (INTEGRATION.md shows
 * the stubs).  Every entry point below names the reference code it replaces (file:line under
 * /root/reference).
 *
 * Conventions
 *   - plain C: raw device pointers, explicit sizes/strides, no torch types;
 *   - all tensors fp32 row-major unless stated; token ids int64 (torch.long) as in the reference;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); calls only enqueue work:
 *     they never allocate, never synchronise, never throw;
 *   - return value: 0 on success, a hipError_t (>0) from the launch, or CAPMI_EINVAL (-1) on bad
 *     arguments.  Nothing here falls back to the CPU.
 */
#ifndef CAPMI_H
#define CAPMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAPMI_EINVAL (-1)
#define CAPMI_MAX_SEG 4
#define CAPMI_MAX_BCOL 3
/* GEMM workspace layout: the first CAPMI_WS_COUNTER_FLOATS 4-byte words are per-tile arrival tickets for
 * the in-launch split-K reduction (must be ZERO when a workspace is first used; kernels re-arm them),
 * K-slice slabs follow.  A fused consumer of deferred slices reads them at partial + this offset. */
#define CAPMI_WS_COUNTER_FLOATS 16384

/* library / device introspection -------------------------------------------------------------- */
int capmi_version(void);                 /* ABI version, bumped on any signature change */
const char *capmi_arch(void);            /* "gfx950" */

/* ---------------------------------------------------------------------------------------------
 * fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32; exact-f32 products, f32 accumulate).
 * Replaces the addmm/mm calls behind nn.Linear / nn.LSTMCell on the hot path:
 *   AttModel.py:118-122 (fc_embed, att_embed, ctx2att), :628/:635 (LSTMCell gate GEMMs),
 *   :733 (h2att), :172 (logit), and their autograd backward (dX = dY W, dW = dY^T X).
 *
 *   C[M,N] = epi( sum_s opA(A_s)[M,K_s] * opB(B_s)[K_s,N] )
 *
 * a_layout: 0 = A_s stored [M][K_s] (row stride lda)      1 = A_s stored [K_s][M] (row stride lda)
 * b_layout: 0 = B_s stored [N][K_s] (nn.Linear weight)    1 = B_s stored [K_s][N]
 * a_row_div: operand row r reads stored row r / a_row_div (image-sharing of per-image activations,
 *            replaces models/utils.py:3-14 repeat_tensors; a_layout 0 only, >= 1).
 * epilogue (applied when the K reduction is complete):
 *   v = acc + bias[n] + bias2[n] + row_bias[(m / row_bias_div) * N + n]
 *   if relu: v = max(v, 0);  if mul_mask: v *= mul_mask[m * N + n];  if accumulate: v += (addend ? addend : C)[m*ldc+n]
 * split-K: splits > 1 writes raw K-slice sums to the workspace `partial` (layout: see
 *   CAPMI_WS_COUNTER_FLOATS; slabs are [splits][M][N]).  Unless defer_reduce, the slices are combined
 *   and the epilogue applied INSIDE the launch by the last-arriving workgroup of each tile (skinny
 *   path) or by a follow-up reduce kernel (fat path).  splits == 0 lets the library choose.
 * ------------------------------------------------------------------------------------------- */
typedef struct capmi_gemm_seg {
    const float *A;
    const float *B;
    int lda;
    int ldb;
    int K;
    int a_row_div;
} capmi_gemm_seg;

typedef struct capmi_gemm_desc {
    capmi_gemm_seg seg[CAPMI_MAX_SEG];
    int nseg;
    int a_layout;
    int b_layout;
    int M;
    int N;
    float *C;
    int ldc;
    const float *bias;
    const float *bias2;
    const float *row_bias;
    int row_bias_div;
    const float *mul_mask;
    int relu;
    int accumulate;
    float *partial;
    int64_t partial_capacity;   /* in floats */
    int splits;                 /* 0 = auto */
    int defer_reduce;           /* leave partials for a fused consumer (e.g. capmi_lstm_cell_fwd) */
    int splits_used;            /* out: number of K slices actually written */
    /* optional (M <= 64 decode GEMMs): segment s's activations ALSO delivered pre-split as "A planes" (see
     * capmi_planes_from_f32); with planes for every segment the loader / consumer kernel stages them by LDS-DMA instead of
     * splitting them inside every workgroup.  Same result bit for bit. */
    const void *a_planes[CAPMI_MAX_SEG];
    /* optional, with accumulate: v += addend[m*ldc+n] instead of C's previous content -- a residual stream that has to stay
     * intact for the backward (x + sublayer(norm(x)), TransformerModel.py:99-102) is added in the epilogue without a copy of it
     * into C first.  Same row pitch as C; may not overlap C. */
    const float *addend;
    /* r6: with defer_reduce, the caller states PER CALL that nothing runs beside this GEMM on another stream, so the planner may give
     * it 256 x 128 tiles (ops.DeferredGrads without its side stream).  The fat GEMMs (bf16x3) run on 128 x 128 or 256 x 128 tiles,
     * whichever the planner costs lower; a 256 x 128 workgroup (16 waves, 144 KB of LDS) owns its CU, so GEMMs whose reduction is
     * DEFERRED -- the weight gradients a trainer may run on a side stream beside its backward chain (train.py:193 `loss.backward()`
     * has no such notion: autograd runs them in line) -- are kept on 128 x 128 tiles while this is 0. */
    int allow_wide_deferred;
    /* r7 (b_layout 1, nseg 1, M <= 64 with A planes: the dX GEMMs of a BPTT step): B delivered as n_bcol column segments that stay
     * where they are -- output columns [sum of bcol_n[0..i), + bcol_n[i]) are A [K][bcol_B[i] with row stride bcol_ldb[i]] -- instead
     * of one matrix packed side by side (dX = dG [W_ih | W_hh] with the two weights read in place).  N = sum of bcol_n; every
     * bcol_n[i] % 4 == 0, 16-byte aligned; seg[0].B / ldb are ignored.  Each output element is the same sum in the same order as
     * with a packed B: bit-identical.  Served by the loader / consumer kernel only (CAPMI_EINVAL where that kernel cannot run).
     * 0: B is seg[].B. */
    int n_bcol;
    const float *bcol_B[CAPMI_MAX_BCOL];
    int bcol_ldb[CAPMI_MAX_BCOL];
    int bcol_n[CAPMI_MAX_BCOL];
} capmi_gemm_desc;

int capmi_gemm_f32(capmi_gemm_desc *d, void *stream);
/* What capmi_gemm_f32 would do with *d, without doing it: the kernel configuration (*route, one of the CAPMI_GEMM_LOG census names:
 * lc, ares_x3, ares_x3_half, ares_f32, t32x128, t64x64, t64x128, t128, x3, x3w, x3w_swap), the K split it would report in splits_used
 * and where the epilogue would be applied (*epi: kernel, reduce or slabs).  Static strings; any out pointer may be NULL.  Host
 * arithmetic over the descriptor only: nothing is launched, no pointer of *d is dereferenced, *d is not written and no device is
 * needed.  CAPMI_EINVAL for exactly the descriptors capmi_gemm_f32 refuses. */
int capmi_gemm_plan(const capmi_gemm_desc *d, const char **route, int *splits, const char **epi);

/* r6: n INDEPENDENT weight-gradient GEMMs in one launch,
 *     C_i [M_i, N_i] (row pitch ldc) (+)= A_i^T B_i,   A_i [K_i, M_i] (pitch lda), B_i [K_i, N_i] (pitch ldb)
 * -- the dW = dY^T X products that autograd's backward (train.py:193 `loss.backward()`; nn.Linear / nn.LSTMCell weight gradients
 * behind AttModel.py:615-640, TransformerModel.py:84-160, AoAModel.py:100-186) produces one by one and that nothing reads before the
 * optimizer.  All their output tiles form ONE persistent grid on the 256 x 128 bf16x3 kernel: the full rounds of the grid write whole-K
 * tiles straight into C, the last partial round is cut into K slices ([256 x 128] pieces in `slabs`, <= 256 of them per launch)
 * that a small second launch sums -- instead of n sub-wave grids with a K split, a slab round trip and a prologue / tail each.
 * The item table travels in the kernel arguments (no device table, no upload: the call is capturable into a hipGraph); more than
 * ~40 items go out as several launches, longest K first.  Items the fat kernel cannot take (M or N not a multiple of 4 -- any K is fine --, unaligned
 * operands / pitches) are issued through capmi_gemm_f32 behind the group.  Same numbers, bit for bit, as capmi_gemm_f32 on each
 * item with the K split reported in splits_used.
 * slabs / slab_floats: scratch for the K-slice pieces (>= 8.4 M floats serves any group; less only limits the tail's K split). */
typedef struct capmi_group_gemm {
    const float *A, *B;
    float *C;
    int32_t lda, ldb, ldc, K, M, N;
    int32_t accumulate;          /* C += instead of C = */
    int32_t splits_used;         /* out: K slices of this item's tail tiles (1 when every tile was written whole-K); -1: went through capmi_gemm_f32 */
    float *colsum;               /* optional: colsum[m] = sum_k A[k, m] -- the BIAS gradient that goes with the weight gradient (nn.Linear:
                                  * db = column sums of dY).  Taken by the staging waves from the A panel they stage anyway instead of a
                                  * second pass over dY (capmi_colsum_batch: 1.0 ms of a Transformer XE step); deterministic (fixed order). */
} capmi_group_gemm;
int capmi_gemm_group_tn(capmi_group_gemm *items, int n, float *slabs, int64_t slab_floats, void *stream);

/* "A planes" of an activation matrix X[M <= 64, K] (row pitch ld): K in chunks of 32, chunk = [3 planes][64 rows][32 bf16],
 * x = h + m + l split exactly into three truncated bf16 values, 16-byte pieces of a row XOR-swizzled by (row >> 2) & 3 -- the
 * LDS image the decode GEMM reads its MFMA fragments from.  The buffer (capmi_planes_bytes(K) bytes, 16-byte aligned) must
 * be zero-filled ONCE when it is allocated: rows >= M and columns >= K are never written.  On the hot path the producers of
 * the activations (capmi_lstm_cell_fwd_pl, capmi_attention_fwd_partial_pl, the select kernel's next-token embedding,
 * capmi_lstm_cell_bwd_partial_pl) write the planes themselves; this call converts any other operand. */
int64_t capmi_planes_bytes(int K);
int capmi_planes_from_f32(const float *X, int ld, int M, int K, void *planes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused additive region attention, forward (AttModel.py:728-748 Attention.forward; the
 * 7-9 ATen launches of SURVEY.md K5 in one kernel):
 *   e[r,k]   = sum_a w[a] * tanh(p_att[r/n, k, a] + att_h[r, a]) + b
 *   alpha    = softmax_k(e);  if mask: alpha = alpha*mask[r/n,k] / sum_k(alpha*mask)
 *   ctx[r,:] = sum_k alpha[r,k] * att[r/n, k, :]
 * One workgroup per image: its p_att / att tiles are read from HBM once and reused by the n rows
 * of that image (no repeat_tensors copy).  att_h [N,A], p_att [B,K,A], att [B,K,R], mask [B,K] or
 * NULL, w [A], b scalar pointer; outputs ctx [N,R], alpha [N,K].  N = B*n, n <= 8.
 * ------------------------------------------------------------------------------------------- */
/* row_img (optional, int32 [N]): explicit row -> image map for ragged groupings (the fused
 * greedy+sample SCST rollout: B*n sampled rows on train-mode features followed by B greedy rows on
 * eval-mode features).  With row_img the call takes N rows (n is ignored) and one row per workgroup. */
int capmi_attention_fwd(const float *att_h, const float *p_att, const float *att, const float *mask,
                        const float *w, const float *b, float *ctx, float *alpha,
                        int B, int n, int K, int A, int R, const int32_t *row_img, int N, void *stream);

/* Same, with att_h delivered as the h2att GEMM's K-slice slabs (capmi_gemm_f32, defer_reduce = 1):
 * att_h[r,:] = sum_{s<h_splits} h_partial[s*h_stride + r*A + :] + h_bias.  The finished rows are also written to
 * att_h_out [N,A] when given (the backward pass needs them). */
int capmi_attention_fwd_partial(const float *h_partial, int h_splits, int64_t h_stride, const float *h_bias,
                                float *att_h_out, const float *p_att, const float *att, const float *mask,
                                const float *w, const float *b, float *ctx, float *alpha,
                                int B, int n, int K, int A, int R, const int32_t *row_img, int N, void *stream);
/* Same; ctx is also written as "A planes" (capmi_planes_from_f32 layout, N <= 64) for the language-LSTM gate GEMM. */
int capmi_attention_fwd_partial_pl(const float *h_partial, int h_splits, int64_t h_stride, const float *h_bias,
                                   float *att_h_out, const float *p_att, const float *att, const float *mask,
                                   const float *w, const float *b, float *ctx, float *alpha,
                                   int B, int n, int K, int A, int R, const int32_t *row_img, int N, void *ctx_planes,
                                   void *stream);

/* backward of the above for one time step.  Inputs d_ctx [N,R] plus the saved att_h/alpha.
 * Outputs d_att_h [N,A] (feeds h2att backward) and d_e [N,K] (softmax-input gradient, kept for the
 * time-batched parameter/feature gradients below). */
int capmi_attention_bwd(const float *d_ctx, int ld_dctx, const float *att_h, const float *alpha,
                        const float *p_att, const float *att, const float *mask, const float *w,
                        float *d_att_h, float *d_e, int B, int n, int K, int A, int R,
                        const int32_t *row_img, int N, void *stream);
/* Same, with d_ctx delivered as the first R of x_cols columns of a dX GEMM left as K-slice slabs (capmi_gemm_f32,
 * defer_reduce = 1): x[r,:] = sum_{s<x_splits} x_slabs[s*x_stride + r*x_cols + :].  Every workgroup finishes the
 * reduction of its rows over all x_cols columns and publishes them to x_out [N, x_cols] (so the LSTM-cell backward and
 * the time-batched pass read finished rows) -- the dX GEMM needs no reduce launch.  x_cols % 4 == 0, 16-byte aligned. */
int capmi_attention_bwd_partial(const float *x_slabs, int x_splits, int64_t x_stride, int x_cols, float *x_out,
                                const float *att_h, const float *alpha, const float *p_att, const float *att,
                                const float *w, float *d_att_h, float *d_e, int B, int n, int K, int A, int R,
                                const int32_t *row_img, int N, void *stream);

/* time-batched feature/parameter gradients of the attention over a whole rollout of T steps:
 *   d_att[b,k,:]   += sum_{t, r in image b} alpha[t,r,k] * d_ctx[t,r,:]
 *   d_p_att[b,k,a] += sum_{t, r in b} d_e[t,r,k] * w[a] * (1 - tanh^2(p_att[b,k,a] + att_h[t,r,a]))
 *   d_w[a]         += sum_{t,r,k} d_e[t,r,k] * tanh(p_att[b,k,a] + att_h[t,r,a]);  d_b += sum d_e
 * All *_all arrays are [T,N_stride,...] (d_ctx_all rows have pitch ld_dctx); image b owns rows
 * b*n .. b*n+n-1 of every time slab (rows >= B*n, e.g. greedy rows, are ignored).  d_att/d_p_att/d_w/d_b
 * are overwritten (not accumulated). */
int capmi_attention_bwd_batched(const float *d_ctx_all, int ld_dctx, const float *att_h_all, const float *alpha_all,
                                const float *d_e_all, const float *p_att, const float *w,
                                float *d_att, float *d_p_att, float *d_w, float *d_b,
                                int T, int B, int n, int N_stride, int K, int A, int R, void *stream);
/* Same; with dw_partial ([B*K, A] floats of scratch) the alpha_net weight gradient is left as one partial row per (image,
 * region) -- d_w = column sum of dw_partial, to be taken by the caller (capmi_colsum / capmi_colsum_batch_args; d_w itself is
 * not touched and may be NULL) -- instead of B*K*A atomicAdds onto A addresses. */
int capmi_attention_bwd_batched_ws(const float *d_ctx_all, int ld_dctx, const float *att_h_all, const float *alpha_all,
                                   const float *d_e_all, const float *p_att, const float *w,
                                   float *d_att, float *d_p_att, float *d_w, float *d_b,
                                   int T, int B, int n, int N_stride, int K, int A, int R, float *dw_partial, void *stream);

/* ---------------------------------------------------------------------------------------------
 * LSTM cell pointwise stage (torch.nn.LSTMCell gate math, gate order i,f,g,o; AttModel.py:628,635):
 *   gates = sum_s partial[s] + b_ih + b_hh + row_bias[(r / row_bias_div)]   ([N,4R])
 *   c' = sig(f)*c + sig(i)*tanh(g);  h' = sig(o)*tanh(c')
 * Consumes the split-K partials of capmi_gemm_f32 directly (defer_reduce).  Writes h', c', the
 * activated gates [N,4R] (saved for backward) and, if out_mask, h_drop = h' * out_mask
 * (F.dropout at AttModel.py:637).
 * ------------------------------------------------------------------------------------------- */
/* row_bias_idx (optional int32 [N]) replaces r / row_bias_div as the row_bias row index. */
int capmi_lstm_cell_fwd(const float *partial, int splits, const float *b_ih, const float *b_hh,
                        const float *row_bias, int row_bias_div, const int32_t *row_bias_idx, const float *c_prev,
                        float *h, float *c, float *gates_act, const float *out_mask, float *h_drop,
                        int N, int R, void *stream);
/* Same; h and / or h_drop are also written as "A planes" (capmi_planes_from_f32 layout, N <= 64, either may be NULL) for the
 * GEMMs that consume them next (h2att + both LSTM gate GEMMs / the vocabulary projection). */
int capmi_lstm_cell_fwd_pl(const float *partial, int splits, const float *b_ih, const float *b_hh,
                           const float *row_bias, int row_bias_div, const int32_t *row_bias_idx, const float *c_prev,
                           float *h, float *c, float *gates_act, const float *out_mask, float *h_drop,
                           int N, int R, void *h_planes, void *h_drop_planes, void *stream);
/* Same; the gate pre-activations are the sum of TWO slab sets (same slab stride N*4R): `partial` and `partial2` (K segments of
 * the gate GEMM computed by separate launches meet here).  splits2 = 0: one set. */
int capmi_lstm_cell_fwd_pl2(const float *partial, int splits, const float *partial2, int splits2, const float *b_ih,
                            const float *b_hh, const float *row_bias, int row_bias_div, const int32_t *row_bias_idx,
                            const float *c_prev, float *h, float *c, float *gates_act, const float *out_mask, float *h_drop,
                            int N, int R, void *h_planes, void *h_drop_planes, void *stream);

/* backward: given dh (total gradient reaching h'), dc_next (gradient reaching c' from step t+1),
 * the saved activated gates, c_prev and c': d_gates [N,4R] (pre-activation) and dc_prev [N,R].
 * dh may be the sum of up to three addends (dh_a + dh_b + dh_c, each optional) and dh_a may be
 * multiplied by a dropout mask first (dropout backward of AttModel.py:637). */
int capmi_lstm_cell_bwd(const float *dh_a, int ld_a, const float *dh_a_mask, const float *dh_b, int ld_b,
                        const float *dh_c, int ld_c, const float *dc_next, const float *gates_act,
                        const float *c_prev, const float *c_new, float *d_gates, float *dc_prev, int N, int R,
                        void *stream);
/* Same, with dh_b and/or dh_c delivered as split-K slabs of the dX GEMMs (capmi_gemm_f32, defer_reduce = 1):
 * dh_b[r,j] = sum_{s<b_splits} dh_b[s*b_stride + r*ld_b + j] (likewise dh_c); splits = 1 is a plain matrix. */
int capmi_lstm_cell_bwd_partial(const float *dh_a, int ld_a, const float *dh_a_mask,
                                const float *dh_b, int ld_b, int b_splits, int64_t b_stride,
                                const float *dh_c, int ld_c, int c_splits, int64_t c_stride,
                                const float *dc_next, const float *gates_act, const float *c_prev,
                                const float *c_new, float *d_gates, float *dc_prev, int N, int R, void *stream);
/* Same; d_gates [N,4R] is also written as "A planes" (N <= 64) for the dX GEMM of the BPTT step. */
int capmi_lstm_cell_bwd_partial_pl(const float *dh_a, int ld_a, const float *dh_a_mask,
                                   const float *dh_b, int ld_b, int b_splits, int64_t b_stride,
                                   const float *dh_c, int ld_c, int c_splits, int64_t c_stride,
                                   const float *dc_next, const float *gates_act, const float *c_prev,
                                   const float *c_new, float *d_gates, float *dc_prev, int N, int R,
                                   void *d_gates_planes, void *stream);

/* token embedding: x[r,:] = relu(E[it[r],:]) * mask[r,:]  (AttModel.py:74-76,168). relu/mask optional. */
/* it[r*it_stride] is row r's token; it_save [N] (optional) records the tokens consumed. */
int capmi_embed_fwd(const int64_t *it, int it_stride, int64_t *it_save, const float *E, const float *mask,
                    float *x, int N, int Edim, int relu, void *stream);
/* Same; x is also written as "A planes" (N <= 64) for the attention-LSTM gate GEMM. */
int capmi_embed_fwd_pl(const int64_t *it, int it_stride, int64_t *it_save, const float *E, const float *mask,
                       float *x, int N, int Edim, int relu, void *x_planes, void *stream);
/* scatter-add backward into dE [V1,Edim] (caller zeroes dE): dE[it[r]] += dx[r]*mask[r]*(x[r]>0) */
int capmi_embed_bwd(const int64_t *it, const float *dx, const float *x_saved, const float *mask,
                    float *dE, int rows, int Edim, int relu, void *stream);

/* ---------------------------------------------------------------------------------------------
 * log-softmax + next-token choice + rollout bookkeeping for one step
 * (F.log_softmax AttModel.py:172; CaptionModel.sample_next_word CaptionModel.py:370-407;
 *  unfinished masking / seq and seqLogprobs stores AttModel.py:340-347).
 *   logits [N,V1] -> logp = logits - logsumexp
 *   mode 0 greedy: first maximal index (torch.max tie-break)
 *   mode 1 sample: argmax_v(logp[v]/temperature + gumbel(v)), gumbel from `gumbel` [N,V1] if given
 *                  else Philox(seed, step, row, v)
 *   mode 2 forced: token = forced[r*forced_ld + step]
 *   step > 0: token *= unfinished[r]; logp row *= unfinished[r]   (finished rows emit pad=0 / zeros)
 *   unfinished[r] = (step==0 ? 1 : unfinished[r]) && token != 0
 *   (mode 2 with no_finish_mask = 1: teacher forcing a_5, nothing is masked)
 * writes seq[r*seq_ld+step], it_next[r], seq_logp[(r*L+step)*V1 + v] (dense, API parity),
 * sel_logp[r*L+step], live[r*L+step] (1 = the row was unfinished when this step was produced).
 * row_mode [N] (optional) overrides `mode` per row (fused greedy+sample).
 * ------------------------------------------------------------------------------------------- */
int capmi_logsoftmax_select(const float *logits, int N, int V1, int step, int L,
                            int mode, const uint8_t *row_mode, float temperature,
                            const float *gumbel, uint64_t seed,
                            const int64_t *forced, int forced_ld, int no_finish_mask,
                            int64_t *seq, int seq_ld, int64_t *it_next, uint8_t *unfinished,
                            float *seq_logp, float *sel_logp, uint8_t *live, void *stream);

/* Optional tail of capmi_logsoftmax_select_partial: the workgroup that chose row r's token also writes the NEXT step's
 * input embedding x[r,:] = relu?(E[token,:]) * mask[r,:] and it_save[r] = token (capmi_embed_fwd of step t+1 folded in). */
typedef struct {
    const float *E;      /* [V1, Edim] embedding table */
    const float *mask;   /* [N, Edim] dropout mask of the next step or NULL */
    float *x;            /* [N, Edim] out; NULL disables the tail */
    int64_t *it_save;    /* [N] or NULL */
    int Edim;
    int relu;
    void *x_planes;      /* optional (N <= 64): the same rows also as "A planes" (capmi_planes_from_f32) for the next gate GEMM */
    int *alive;          /* optional, independent of x: every row that is still unfinished after this step stores 1 here (device-
                          * visible memory, e.g. pinned host memory: the rollout driver's early exit, AttModel.py:349-350) */
} capmi_next_embed;

/* Optional top-k / nucleus filter of the sampling modes (CaptionModel.sample_next_word, CaptionModel.py:388-404,
 * sample_method 'top<k>' / 'top<p>'): only the top_k most probable tokens, or the smallest set of most probable tokens
 * whose probability (softmax of logp / temperature) reaches top_p, can be drawn.  At most one of the two is non-zero. */
typedef struct {
    int top_k;      /* 0 = off */
    float top_p;    /* 0 = off, else in (0,1) */
} capmi_sample_filter;

/* Same, fed straight from the vocabulary GEMM's K-slice slabs (capmi_gemm_f32 with defer_reduce = 1):
 * logits[r,:] = sum_{s<splits} partial[s*slab_stride + r*V1 + :] + bias (bias may be NULL).  With V1 % 4 == 0,
 * V1 <= 12288 and 16-byte aligned buffers the row lives in registers (no split-K reduce launch, no logits
 * round trip); any other size / alignment runs a streaming kernel that re-assembles the row per pass. */
/* mode flag of the select entry points (OR it into `mode`): store the row of LOGITS (slabs + bias) in seq_logp / sel_logp instead of
 * the log-probabilities -- AttModel.get_logprobs_state(output_logsoftmax=0), AttModel.py:171-175, used by the margin structure losses
 * (loss_wrapper.py:31-37).  The choice of the token is unaffected (arg-max / Gumbel-max are shift invariant). */
#define CAPMI_SELECT_RAW 256
int capmi_logsoftmax_select_partial(const float *partial, int splits, int64_t slab_stride, const float *bias,
                                    int N, int V1, int step, int L,
                                    int mode, const uint8_t *row_mode, float temperature,
                                    const float *gumbel, uint64_t seed,
                                    const int64_t *forced, int forced_ld, int no_finish_mask,
                                    int64_t *seq, int seq_ld, int64_t *it_next, uint8_t *unfinished,
                                    float *seq_logp, float *sel_logp, uint8_t *live,
                                    const capmi_next_embed *next, const capmi_sample_filter *filter, void *stream);
/* r4: the same select with a GEMM riding in the idle workgroups of ITS launch.  `ahead` describes a loader / consumer decode GEMM
 * (M <= 64, every segment with A planes, defer_reduce = 1: K-slice slabs in ahead->partial, ahead->splits_used on return) that
 * depends on nothing this select writes -- in the rollout: the h_lang / h_att segments of the NEXT step's attention-LSTM gates
 * (AttModel.py:626-627), 2/3 of that GEMM's weights.  N select workgroups + the GEMM's workgroups must fit 256; when they do
 * not, or the GEMM / select take another kernel, both are launched one after the other with identical results. */
int capmi_logsoftmax_select_partial_gemm(const float *partial, int splits, int64_t slab_stride, const float *bias, int N,
                                         int V1, int step, int L, int mode, const uint8_t *row_mode, float temperature,
                                         const float *gumbel, uint64_t seed, const int64_t *forced, int forced_ld,
                                         int no_finish_mask, int64_t *seq, int seq_ld, int64_t *it_next, uint8_t *unfinished,
                                         float *seq_logp, float *sel_logp, uint8_t *live, const capmi_next_embed *next,
                                         const capmi_sample_filter *filter, capmi_gemm_desc *ahead, void *stream);

/* gradient of the dense log-probs w.r.t. the logits for ALL steps at once:
 *   dlogits[r,t,:] = g[r,t,:] - exp(logp[r,t,:]) * sum_v g[r,t,v]      (rows where logp was masked
 *   to zero receive zero: `live` [N,L] uint8, 1 = the row was live when step t was produced) */
/* g, seq_logp are [N,L,V1]; only steps t < T are produced; dlogits is written TIME-MAJOR
 * [T,N,V1] so that it lines up with the saved [T,N,...] activations for the batched GEMMs. */
int capmi_logsoftmax_bwd(const float *g, const float *seq_logp, const uint8_t *live, float *dlogits,
                         int N, int L, int T, int V1, void *stream);

/* Sparse form of the same gradient: every criterion of the hot path reads the dense
 * log-probs only through ONE entry per (row, step) -- `input.gather(2, target)` at losses.py:24 (RewardCriterion), :81
 * (StructureLosses), :213 (LanguageModelCriterion) -- and, for LabelSmoothing (:258-262), through the row sum.  With
 *   g_sel [N,L] = dL / d logp[r,t,tok[r,t]]   (NULL: none)      tok [N,tok_ld] int64, tok_ld >= T
 *   g_sum [N,L] = dL / d sum_v logp[r,t,v]    (NULL: none)
 * the gradient w.r.t. the logits is  g_sel (onehot(tok) - p) + g_sum (1 - V1 p),  p = exp(logp); an additional dense
 * gradient `g` [N,L,V1] (NULL: none) is added in its dense form.  The [N,L,V1] gradient tensor of the reference's autograd
 * (zero fill + scatter) is never materialised. */
typedef struct capmi_sparse_logp_grad {
    const float *g_sel;
    const float *g_sum;
    const int64_t *tok;
    int tok_ld;
    int raw;              /* r4: 1 = the rollout returned the raw logits (CAPMI_SELECT_RAW, output_logsoftmax = 0): d(logits) is the loss
                           * gradient itself -- g_sel at the token, g_sum everywhere, plus the dense g -- without the softmax Jacobian */
    const float *scale;   /* NULL, or a DEVICE scalar multiplying g_sel / g_sum (the upstream gradient of a scalar loss) */
} capmi_sparse_logp_grad;
int capmi_logsoftmax_bwd_sparse(const capmi_sparse_logp_grad *sp, const float *g, const float *seq_logp,
                                const uint8_t *live, float *dlogits, int N, int L, int T, int V1, void *stream);

/* RewardCriterion.forward (losses.py:18-37) on the selected log-probs a rollout wrote (capmi_updown_rollout.sel_logp):
 *   mask[r,t] = 1 for t == 0, else (seq[r,t-1] > 0)            (the EOS step still counts, losses.py:28-29)
 *   loss = -sum(sel * reward * mask) / sum(mask)                 (per_row: one value per row, reduction='none')
 *   gcoef[r,t] = d loss / d sel[r,t]  (rows N_used .. N_all-1, e.g. the greedy rows of a fused SCST rollout: 0)
 * reward[r,t] is read at reward[r * reward_row_stride + t * reward_col_stride] ([N] advantage: strides 1, 0). */
int capmi_reward_criterion(const float *sel, int sel_ld, const int64_t *seq, int seq_ld, const float *reward,
                           int reward_row_stride, int reward_col_stride, int N_used, int N_all, int L, int per_row,
                           float *loss, float *gcoef, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Elementwise helpers
 * ------------------------------------------------------------------------------------------- */
/* out = sum_s partial[s] (+bias +bias2) then relu / mask (split-K reduce with the GEMM epilogue) */
int capmi_splitk_reduce(const float *partial, int splits, float *C, int ldc, int M, int N,
                        const float *bias, const float *bias2, const float *row_bias, int row_bias_div,
                        const float *mul_mask, int relu, int accumulate, void *stream);
/* The same for MANY independent GEMMs in one launch: the weight-gradient GEMMs of a layer-by-layer backward (dW = dY^T X of
 * every nn.Linear, TransformerModel.py / AoAModel.py) leave their K-slice slabs (capmi_gemm_desc.defer_reduce = 1, one
 * workspace region each) and nothing reads dW before the optimizer, so ONE launch at the end of the backward finishes them
 * all.  `items` is DEVICE memory (the kernel reads the table); slabs of item i: partial + s * M * N, s < splits. */
typedef struct capmi_reduce_item {
    const float *partial;
    float *C;
    const float *bias;
    int32_t splits, M, N, ldc, accumulate, reserved;
} capmi_reduce_item;
int capmi_splitk_reduce_batch(const capmi_reduce_item *items, int n_items, void *stream);
/* Bernoulli keep-masks scaled by 1/(1-p): mask[i] in {0, 1/(1-p)}; Philox4x32-10(seed, offset+i) */
int capmi_dropout_mask(float *mask, int64_t count, float p, uint64_t seed, uint64_t offset, void *stream);
/* up to CAPMI_MAX_MASKS masks in one launch (the fc / att / xt / output dropouts of one rollout, AttModel.py:83-90, 122,
 * 640).  Viewing mask i as slabs of `rows` rows of `row_len` floats, rows >= keep_from are written as 1.0 (eval-mode rows of
 * the fused SCST rollout); rows == 0 or keep_from < 0: none. */
#define CAPMI_MAX_MASKS 4
typedef struct capmi_mask_desc {
    float *mask;
    int64_t count;
    uint64_t offset;
    int row_len, rows, keep_from;
} capmi_mask_desc;
int capmi_dropout_masks(const capmi_mask_desc *descs, int n, float p, uint64_t seed, void *stream);
/* zero `count` floats of up to four state buffers (h1 / c1 may be NULL), it[0..N) = 0 (BOS), unfinished[0..N) = 1:
 * the initial state of AttModel._sample / _forward (init_hidden AttModel.py:99-102, :281-285) in one launch */
int capmi_rollout_init(float *h0, float *c0, float *h1, float *c1, int64_t count, int64_t *it, uint8_t *unfinished, int N,
                       void *stream);
/* out[c] = sum_r in[r*ld + c]  (bias gradients) ; accumulate optional */
int capmi_colsum(const float *in, int rows, int cols, int ld, float *out, int accumulate, void *stream);
/* all bias gradients of a backward in one launch (no atomics, no zero-fill): `items` is DEVICE memory */
typedef struct capmi_colsum_item {
    const float *in;
    float *out;
    float *out2;                 /* optional second copy of the result (nn.LSTMCell's bias_hh gradient = bias_ih's) */
    int32_t rows, cols, ld, accumulate;
} capmi_colsum_item;
int capmi_colsum_batch(const capmi_colsum_item *items, int n_items, void *stream);
/* the same with the items in HOST memory (<= CAPMI_COLSUM_ARGS_MAX of them, passed to the kernel by value) */
#define CAPMI_COLSUM_ARGS_MAX 8
int capmi_colsum_batch_args(const capmi_colsum_item *host_items, int n_items, void *stream);
/* out[g, c] = sum_{j<group} in[(g*group + j)*cols + c], summed over T slabs of stride slab */
int capmi_group_rowsum(const float *in, int T, int64_t slab, int groups, int group, int cols,
                       float *out, void *stream);
/* y = x * (m ? m : 1) * (gate_on_positive && ref<=0 ? 0 : 1): relu/dropout backward */
int capmi_relu_mask_bwd(const float *dy, const float *y_ref, const float *mask, float *dx, int64_t count,
                        void *stream);
/* the same Jacobian when y_ref is the layer's output AFTER its dropout mask (y = relu(pre) * mask, the fused epilogue of the
 * forward GEMM; nn.Sequential(Linear, ReLU, Dropout): AttModel.py:83-90, TransformerModel.py:215 PositionwiseFeedForward): y > 0
 * exactly where mask and ReLU both passed, and there mask == 1 / (1 - p) == scale -- the mask tensor is not read.
 * count % 4 == 0, 16-byte aligned operands. */
int capmi_relu_scale_bwd(const float *dy, const float *y_ref, float scale, float *dx, int64_t count, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused value-clip + Adam on one flat fp32 buffer (torch.nn.utils.clip_grad_value_ train.py:194-195
 * + torch.optim.Adam misc.py:125-126; the flat buffer is also what the single RCCL all-reduce moves).
 *   g = clamp(g * grad_scale, -clip, clip) (clip <= 0: none);  m,v,p updated with bias correction.
 * ------------------------------------------------------------------------------------------- */
int capmi_adam_step(float *p, const float *g, float *m, float *v, int64_t count, float lr, float beta1,
                    float beta2, float eps, float weight_decay, float clip, float grad_scale, int step,
                    void *stream);

/* ---------------------------------------------------------------------------------------------
 * Per-step state in DEVICE memory, so that a whole training iteration (tools/train.py:185-196: forward, loss, backward,
 * clip + Adam) can be captured ONCE into a hipGraph and replayed: what changes from one iteration to the next -- the
 * dropout / sampling random stream and Adam's step count (bias corrections) and learning rate -- is read from this record
 * by the kernels instead of arriving as kernel arguments, which a graph would freeze.
 *   capmi_step_advance   one thread: epoch += 1; adam_step += 1; bc1 = 1 - beta1^adam_step; bc2_sqrt = sqrt(1 - beta2^adam_step)
 *                        (double arithmetic, like capmi_adam_step does on the host).  First launch of every iteration.
 *   capmi_step_set_lr    lr = value (launched outside the graph, when the schedule changes it: misc.py set_lr)
 *   capmi_rng_bind_epoch every kernel that takes a Philox `seed` (dropout masks, token sampling) uses
 *                        seed + 0x9E3779B97F4A7C15 * (*epoch) while a non-NULL epoch pointer is bound (process-wide; one
 *                        process per GPU).  NULL (the default) = the seed argument alone, as before.  Returns the
 *                        previous binding through *prev when prev != NULL.
 *   capmi_adam_step_dyn  capmi_adam_step with lr, bc1, bc2_sqrt read from the record.
 * ------------------------------------------------------------------------------------------- */
typedef struct capmi_step_state {
    uint64_t epoch;
    int32_t adam_step;
    float lr, bc1, bc2_sqrt;
    float reserved[2];
} capmi_step_state;
/* hipMemcpyAsync host -> device on `stream` from PINNED host memory the caller keeps alive and unchanged (inside a graph capture
 * this becomes a memcpy node that re-reads `src` at every replay: the item tables of capmi_splitk_reduce_batch /
 * capmi_colsum_batch of a captured backward). */
int capmi_upload_async(void *dst, const void *src_pinned, int64_t bytes, void *stream);
int capmi_step_advance(capmi_step_state *state, float beta1, float beta2, void *stream);
int capmi_step_set_lr(capmi_step_state *state, float lr, void *stream);
int capmi_rng_bind_epoch(const uint64_t *epoch, const uint64_t **prev);
int capmi_adam_step_dyn(float *p, const float *g, float *m, float *v, int64_t count, const capmi_step_state *state,
                        float beta1, float beta2, float eps, float weight_decay, float clip, float grad_scale,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * The other rules of misc.build_optimizer (misc.py:114-130) on the flat fp32 buffer, fused with the same pre-processing as
 * capmi_adam_step: g = clamp(g * grad_scale, -clip, clip) (clip <= 0: none).  One launch, every stream read and written once.
 *   CAPMI_OPTIM_RMSPROP  torch.optim.RMSprop(lr, alpha, eps, weight_decay): g += wd p; s1 = alpha s1 + (1 - alpha) g^2;
 *                        p -= lr g / (sqrt(s1) + eps)                                                    s1 = 'square_avg'
 *   CAPMI_OPTIM_ADAGRAD  torch.optim.Adagrad(lr, weight_decay), lr_decay 0: g += wd p; s1 += g^2;
 *                        p -= lr g / (sqrt(s1) + eps)   (the caller passes torch's default eps, 1e-10)   s1 = 'sum'
 *   CAPMI_OPTIM_SGDM     torch.optim.SGD(lr, momentum = alpha, weight_decay): g += wd p; s1 = step == 1 ? g : alpha s1 + g;
 *                        p -= lr s1                                                                      s1 = 'momentum_buffer'
 *   CAPMI_OPTIM_SGDMOM   the same with nesterov=True: p -= lr (g + alpha s1)
 *   CAPMI_OPTIM_ADAMW    torch.optim.AdamW(lr, (alpha, beta), eps, weight_decay): p *= 1 - lr wd; then Adam's update with no L2
 *                        term in g                                                    s1 = 'exp_avg', s2 = 'exp_avg_sq'
 * s2 is read and written by CAPMI_OPTIM_ADAMW only; the other rules never touch it (pass NULL).  p, g, s1 (and s2) need 4-byte
 * alignment only: a range that starts off a 16-byte boundary (a shard of the flat buffer) gets a scalar head and tail.
 *   capmi_optim_step      lr and the 1-based step number by value.
 *   capmi_optim_step_dyn  lr, the step number (capmi_step_state.adam_step, for the first-step rule) and AdamW's bias corrections
 *                         from the device record: capmi_step_advance(state, alpha, beta) and capmi_step_set_lr serve every rule.
 * CAPMI_EINVAL: a NULL hp / p / g / s1 / state (s2 for AdamW), count <= 0, step < 1, an unknown rule, a pointer off 4 bytes.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_OPTIM_RMSPROP 1
#define CAPMI_OPTIM_ADAGRAD 2
#define CAPMI_OPTIM_SGDM 3
#define CAPMI_OPTIM_SGDMOM 4
#define CAPMI_OPTIM_ADAMW 5
typedef struct capmi_optim_hp {
    int32_t rule;           /* CAPMI_OPTIM_* */
    float alpha;            /* rmsprop: smoothing constant; sgdm / sgdmom: momentum; adamw: beta1 */
    float beta;             /* adamw: beta2 */
    float eps;
    float weight_decay;
    float clip;
    float grad_scale;
} capmi_optim_hp;
int capmi_optim_step(const capmi_optim_hp *hp, float *p, const float *g, float *s1, float *s2, int64_t count, float lr,
                     int step, void *stream);
int capmi_optim_step_dyn(const capmi_optim_hp *hp, float *p, const float *g, float *s1, float *s2, int64_t count,
                         const capmi_step_state *state, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Exponential moving average of the flat fp32 parameters (--ema_decay), one launch after the optimizer's, under every rule:
 *   d   = warmup ? min(decay, (1 + step) / (10 + step)) : decay        (float arithmetic, inside the kernel)
 *   ema = fma(d, ema, (1 - d) * p)
 * p is read only; ema is read once and written once (non-temporal: nothing reads the average before the next step).  12 bytes
 * per element.  ema and p need 4-byte alignment only: a range that starts off a 16-byte boundary gets a scalar head and tail,
 * ranges misaligned differently from each other run scalar.
 *   capmi_ema_step      the 1-based step number by value.
 *   capmi_ema_step_dyn  the step number from the device record (capmi_step_state.adam_step, after capmi_step_advance): the
 *                       form a captured training step replays.  Same arithmetic on the same floats: bit-equal.
 * CAPMI_EINVAL, before anything is launched: a NULL ema / p / state, count <= 0, step < 1, decay outside [0, 1), a pointer
 * off 4 bytes, ema == p.
 * ------------------------------------------------------------------------------------------- */
int capmi_ema_step(float *ema, const float *p, int64_t count, float decay, int warmup, int step, void *stream);
int capmi_ema_step_dyn(float *ema, const float *p, int64_t count, const capmi_step_state *state, float decay, int warmup,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * CIDEr-D reward (external pyciderevalcap.ciderD -- see oracle/ciderd.py for the provenance note;
 * call sites rewards.py:41-81, 83-114).  float64 arithmetic on device.
 *   table: open-addressing hash of the document-frequency pickle; keys = n-gram of <= 4 token ids
 *          packed as 4 x 16-bit (id+1), vals = document count (double); capacity power of two;
 *          empty slot key = 0.
 *   hyp   [H, L] int64 token rows (cut after the first 0, which is kept: rewards.py:33-39)
 *   refs  [B, max_refs, ref_w] int32, n_refs [B]; hypothesis h scores against image hyp_img[h];
 *          a negative entry ends a reference WITHOUT an EOS token (a completely filled row of a narrower
 *          source array padded to ref_w: the zero padding must not read as its terminating 0)
 *   scores[H] double = 10 * mean_k( sum_refs sim_k ) / n_refs
 * ------------------------------------------------------------------------------------------- */
int capmi_ciderd_score(const int64_t *hyp, int H, int L, const int32_t *hyp_img,
                       const int32_t *refs, const int32_t *n_refs, int max_refs, int ref_w,
                       const uint64_t *table_keys, const double *table_vals, uint32_t table_cap,
                       double log_ref_len, double *scores, void *stream);
/* References cooked once per batch: n-gram keys, tf-idf vectors, norms and length of every reference of
 * every image, CAPMI_CIDERD_COOKED_BYTES per (image, reference slot) in `cooked` [B * max_refs]; capmi_ciderd_score_cooked
 * then scores hypotheses against them without re-cooking a reference per hypothesis (same arithmetic, same results). */
#define CAPMI_CIDERD_COOKED_BYTES 4392
int capmi_ciderd_cook_refs(const int32_t *refs, const int32_t *n_refs, int B, int max_refs, int ref_w,
                           const uint64_t *table_keys, const double *table_vals, uint32_t table_cap,
                           double log_ref_len, void *cooked, void *stream);
int capmi_ciderd_score_cooked(const int64_t *hyp, int H, int L, const int32_t *hyp_img, const void *cooked,
                              const int32_t *n_refs, int max_refs, const uint64_t *table_keys,
                              const double *table_vals, uint32_t table_cap, double log_ref_len, double *scores,
                              void *stream);
/* advantage + broadcast (rewards.py:76-79): reward[r] = scores[r] - scores[N + r/n]  (float32 [N]) */
int capmi_scst_advantage(const double *scores, int N, int n, float *reward, void *stream);
/* same; mean_out[0] = mean of reward[0..N) (what LossWrapper reports as out['reward'], loss_wrapper.py:72) in the same launch */
int capmi_scst_advantage_mean(const double *scores, int N, int n, float *reward, float *mean_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sentence BLEU-4 and self-CIDEr as training rewards (bleu_reward_weight: rewards.py:68-74, 105-112; self_cider_reward_weight:
 * rewards.py:116-136 used by losses.py:175-182).  coco-caption and the cider submodule are not part of the reference checkout:
 * PARITY UNPINNED, restated in tests/rewards_ref64.py.  Token rows follow the convention of capmi_ciderd_score (cut AFTER the
 * first 0, which is a word; a negative entry ends a reference without one), not that of capmi_langeval.  Double throughout; no
 * allocation, no host sync, no atomics: the same bits on every run.
 *
 * capmi_reward_bleu4: one launch, one workgroup per row of hyp [H, L] against the references of image hyp_img[h] (refs
 *   [B, max_refs, ref_w] int32, n_refs [B], as for capmi_ciderd_score; an image index outside [0, B) has no references).
 *   bleu4 = bleu_scorer's per-sentence Bleu_4, option 'closest' (ties to the shorter reference): p_k = (correct_k + 1e-15) /
 *   (guess_k + 1e-9) with the clipped counts of order k, (p_1 p_2 p_3 p_4)^(1/4), times exp(1 - 1/ratio) when ratio =
 *   (len + 1e-15) / (reflen + 1e-9) < 1.  scores[h] = cw * base[h] + bw * bleu4, or bw * bleu4 when base is NULL; base may be
 *   `scores` itself (the CIDEr-D scores mixed in place).  stats [H, 10] int32, when not NULL, receives guess_1..4, correct_1..4,
 *   len, reflen.  CAPMI_EINVAL: a NULL pointer, L or ref_w outside 1..64, H, B or max_refs
 *   < 1.  Token ids must be below 65535, as for capmi_ciderd_score.
 * capmi_self_cider_reward: two launches over hyp [B * n, L], rows g*n .. g*n+n-1 the samples of image g, 2 <= n <=
 *   CAPMI_SELF_CIDER_NMAX.  K[i][j] = 10 * (1/4) sum_k cos_k on vectors tf * (log_ref_len - log(max(1, df))) with df from the table
 *   of capmi_ciderd_score (an order with a zero norm contributes 0; i <= j computed, mirrored); lambda = eigenvalues of K/10 by
 *   the cyclic Jacobi of capmi_diveval_add, clipped at 0; scores[g] = -log(sqrt(lambda_max) / sum sqrt(lambda)) / log(n), and 0.0
 *   where the sum is 0 (numpy gives NaN).  A weight below 1e-12 in magnitude is 0: an n-gram of every image must weigh
 *   exactly 0 although log_ref_len is the host's logarithm.  Scratch: norm [B * n, 4], dots [B * n, n, 4] doubles.  K [B, n, n] and eig [B, n]
 *   (ascending) are written when not NULL.  CAPMI_EINVAL: a NULL pointer, n or L out of range, B < 1, an invalid table.
 * capmi_nsc_advantage: one launch.  reward[r] = (float)scores[r]; adv[r] = reward[r] - (sum of the image's other n-1 rewards) /
 *   (n - 1) + (float)add_w * (float)add[r / n]  (float32 arithmetic in the order of losses.py:175-182; add may be NULL).
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_SELF_CIDER_NMAX 32
int capmi_reward_bleu4(const int64_t *hyp, int H, int L, const int32_t *hyp_img, const int32_t *refs, const int32_t *n_refs, int B,
                       int max_refs, int ref_w, const double *base, double cw, double bw, double *scores, int32_t *stats,
                       void *stream);
int capmi_self_cider_reward(const int64_t *hyp, int B, int n, int L, const uint64_t *table_keys, const double *table_vals,
                            uint32_t table_cap, double log_ref_len, double *norm, double *dots, double *scores, double *K,
                            double *eig, void *stream);
int capmi_nsc_advantage(const double *scores, const double *add, double add_w, int N, int n, float *reward, float *adv,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * Consensus (minimum-Bayes-risk) reranking of the n candidate captions of an image (opt['rerank'], imagecaptioning/pytorch_amd/
 * mbr.py; not part of the reference): keep the candidate whose expected utility against the other candidates is highest.  hyp
 * [B * n, L] int64, rows g*n .. g*n+n-1 the candidates of image g, 2 <= n <= CAPMI_SELF_CIDER_NMAX, L in 1..64.  Token rows follow
 * the convention of capmi_ciderd_score (cut AFTER the first 0, which is a word); a completely filled row has no end token and, read
 * as a reference, behaves like a reference ended by a negative entry.  Double throughout; no allocation, no host sync, no
 * atomics: the same bits on every run.
 *
 * capmi_mbr_utility: three launches.  U[g][i][j] = the utility of candidate i, read as the hypothesis, against candidate j read as
 *   its only reference (not symmetric; the diagonal is written, nothing downstream reads it).
 *     CAPMI_MBR_CIDERD  the arithmetic of capmi_ciderd_score with n_refs = 1: clipped counts, Gaussian length term, factor 10,
 *                       weights tf * (log_ref_len - log(max(1, df))) on the table of capmi_ciderd_score.
 *     CAPMI_MBR_BLEU4   the bleu4 of capmi_reward_bleu4 with that one reference; takes no table (the pointers may be NULL).
 *   Every candidate is cooked once (n-gram keys, weights, norms, length: the record of capmi_ciderd_cook_refs), then the n * n
 *   pairs of every image are scored, one workgroup each.  scratch: CAPMI_CIDERD_COOKED_BYTES * B * n bytes, 8-byte aligned.
 * capmi_mbr_select: one launch.  expected[g][i] = sum_{j != i} w_j U[g][i][j] / sum_{j != i} w_j, j ascending (0 where that
 *   denominator is 0); w_j = 1 when seq_weight is NULL, else exp(seq_weight[g*n+j] - max over the image), the largest exactly 1
 *   (seq_weight: a log-prior of each candidate, e.g. the sum of its selected log-probs).  A candidate whose caption (the tokens up
 *   to and including the first 0) repeats that of an earlier candidate of its image is never chosen but still counts as a
 *   reference: identical captions have identical rows of U up to the order of the sums, and this rule makes the choice among
 *   them deterministic.  choice[g] = the lowest index with the largest expected value among the first occurrences; 0 when all
 *   expected values are 0.
 * CAPMI_EINVAL, before anything is launched: a NULL pointer (table pointers only for CAPMI_MBR_CIDERD, seq_weight never), B < 1, n
 *   or L out of range, an unknown kind, a table size that is no power of two, a misaligned scratch.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_MBR_CIDERD 0
#define CAPMI_MBR_BLEU4 1
int capmi_mbr_utility(const int64_t *hyp, int B, int n, int L, int kind, const uint64_t *table_keys, const double *table_vals,
                      uint32_t table_cap, double log_ref_len, void *scratch, double *U, void *stream);
int capmi_mbr_select(const double *U, const double *seq_weight, const int64_t *hyp, int B, int n, int L, double *expected,
                     int32_t *choice, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Launch instrumentation (counterpart of the reference's `time/batch` prints, train.py:198-208).
 * capmi_prof_enable(class_mask): launches of the selected kernel classes carry a HIP event pair in the
 * dispatch itself (hipExtLaunchKernelGGL start/stop events on the kernel's own stream: no extra queue
 * packets, negligible perturbation) and their algorithmic bytes/flops are accumulated; read returns the
 * totals of one class.  Classes with in-dispatch events: 0 decode GEMM (M <= 64, x W^T), 1 BPTT GEMM
 * (M <= 64, dG W), 2 fat GEMM, 3 attention fwd, 4 attention bwd.  capmi_prof_read synchronises on the
 * recorded events.
 * ------------------------------------------------------------------------------------------- */
int capmi_prof_enable(int class_mask);
int capmi_prof_reset(void);
int capmi_prof_read(int cls, double *total_ms, int64_t *launches, double *bytes, double *flops);

/* ---------------------------------------------------------------------------------------------
 * Whole-rollout drivers for the UpDown decoder (AttModel._sample AttModel.py:258-352 and
 * AttModel._forward :126-164 with UpDownCore :615-640).  One host call enqueues every kernel of all
 * T steps on `stream` with no host synchronisation: the reference's per-step
 * `.sum()==0` syncs are replaced by on-device finished flags.
 * ------------------------------------------------------------------------------------------- */
typedef struct capmi_updown_weights {
    const float *embed;                                /* [V1,E]   embed.0.weight */
    const float *att_w_ih, *att_w_hh, *att_b_ih, *att_b_hh;   /* core.att_lstm.*  [4R,2R+E],[4R,R] */
    const float *lang_w_ih, *lang_w_hh, *lang_b_ih, *lang_b_hh; /* core.lang_lstm.* [4R,2R],[4R,R] */
    const float *h2att_w, *h2att_b;                    /* [A,R],[A] */
    const float *alpha_w, *alpha_b;                    /* [A],[1]   */
    const float *logit_w, *logit_b;                    /* [V1,R],[V1] */
} capmi_updown_weights;

typedef struct capmi_updown_rollout {
    /* sizes: B images carry gradients and own rows b*n..b*n+n-1; B_feat >= B feature images exist in
     * fc/att/p_att (B_feat > B only with row_img); N rows in total (N == B*n unless row_img is given) */
    int B, n, N, K, A, R, E, V1;
    int B_feat;
    const int32_t *row_img; /* [N] row -> feature image, or NULL (= row / n) */
    int T;                  /* steps to run */
    int L;                  /* step pitch of seq / seq_logp / sel_logp / live (>= T) */
    /* per-image prepared features (outputs of the prefill GEMMs) */
    const float *fc;        /* [B,R]   */
    const float *att;       /* [B,K,R] */
    const float *p_att;     /* [B,K,A] */
    const float *att_mask;  /* [B,K] or NULL */
    /* randomness / control */
    const float *drop_xt;   /* [T,N,E] pre-scaled keep masks or NULL (eval) */
    const float *drop_out;  /* [T,N,R] or NULL */
    int mode;               /* 0 greedy, 1 sample, 2 forced */
    const uint8_t *row_mode;/* optional per-row override */
    float temperature;
    const float *gumbel;    /* [T,N,V1] injected noise or NULL (=> Philox(seed)) */
    uint64_t seed;
    const int64_t *forced;  /* [N, forced_ld] */
    int forced_ld;
    int teacher;            /* 1: _forward semantics: inputs are forced[:,t], nothing masked */
    /* state + saved activations, all [T+1,N,R] with slot 0 = initial zeros */
    float *h_att, *c_att, *h_lang, *c_lang;
    float *xt;              /* [T,N,E]  */
    int64_t *it_all;        /* [T,N]    token fed at each step */
    float *gates_att;       /* [T,N,4R] activated */
    float *gates_lang;      /* [T,N,4R] */
    float *att_h;           /* [T,N,A]  */
    float *alpha;           /* [T,N,K]  */
    float *ctx;             /* [T,N,R]  */
    float *h_drop;          /* [T,N,R]  h_lang after dropout (logit input) */
    /* outputs */
    int64_t *seq;           /* [N,L]   */
    float *seq_logp;        /* [N,L,V1] dense */
    float *sel_logp;        /* [N,L]   */
    uint8_t *live;          /* [N,L]   1 if row was unfinished when step t was computed */
    /* scratch */
    float *fc_gates;        /* [B,4R]  fc-term of the attention LSTM, computed once */
    float *logits;          /* [N,V1]  */
    int64_t *it;            /* [N]     */
    uint8_t *unfinished;    /* [N]     */
    float *partial;         /* split-K workspace */
    int64_t partial_capacity;
    /* sampling filter (mode 1 rows only): see capmi_sample_filter */
    int top_k;
    float top_p;
    /* scheduled sampling (teacher == 1 only; AttModel.py:145-154): [T,N] or NULL.  ss_mode[t*N + r] says where the INPUT
     * token of row r at step t comes from: 2 = forced[r, t] (teacher forcing), 1 = a draw from the model's own distribution
     * of step t-1 (torch.multinomial(exp(outputs[:, t-1])), here Gumbel-max at temperature 1).  Row t = 0 is ignored (BOS). */
    const uint8_t *ss_mode;
    /* Round 3, optional (N <= 64): scratch for the "A planes" of the step's activations (h_att, h_lang, ctx, xt, h_drop + a zero
     * image; capmi_updown_planes_bytes(R, E) bytes, 16-byte aligned, ZERO-FILLED ONCE by the caller when it is allocated and
     * reusable by later rollouts of the same R / E).  With it the producers of the activations write the bf16x3 planes the
     * gate / logit GEMMs stage by LDS-DMA (capmi_gemm_desc.a_planes); NULL keeps the in-GEMM split.  Same results. */
    void *planes;
    int64_t planes_bytes;
    /* Round 3: early exit of free-running rollouts (AttModel.py:349-350 `if unfinished.sum() == 0: break`).  early_exit = k > 0:
     * after every k-th step (from step early_exit_from on) the driver looks, two steps later and through an event, at a word of
     * `alive_host` ([L] int32 of PINNED HOST memory the device can write: the select kernel of step t stores 1 in alive_host[t]
     * for every row that goes on) and stops enqueuing when no row is left.  The steps that were queued behind the decisive one
     * run on finished rows only and write what the reference leaves behind the break (pad tokens, zero log-probs); the
     * log-probs of the steps never run are zero-filled.  steps_run (out) = steps enqueued; the backward then takes
     * r->T = steps_run.  0 / NULL: all T steps are enqueued without any host wait. */
    int early_exit;
    int early_exit_from;
    int32_t *alive_host;
    int steps_run;
    /* r4, optional (needs `planes`, free-running rollouts): K-slice slab workspace (pre_capacity floats, laid out like `partial`:
     * CAPMI_WS_COUNTER_FLOATS zeroed words + slabs) of the AHEAD part of the attention-LSTM gate GEMM.  The K segments fed by
     * h_lang(t) and h_att(t) -- 2/3 of the next step's gate GEMM, independent of the token being chosen -- are computed inside the
     * select launch of step t (capmi_logsoftmax_select_partial_gemm: the select keeps 60 of 256 CUs busy); the gate GEMM of
     * step t+1 keeps the token-embedding segment and the LSTM cell sums both slab sets.  NULL: one gate GEMM per step. */
    float *pre_partial;
    int64_t pre_capacity;
    /* r4: 1 = free-running rollouts return the raw logits in seq_logp / sel_logp (AttModel._sample with output_logsoftmax = 0,
     * AttModel.py:265, 292: the margin structure losses); the backward then takes the loss gradient as d(logits).  Teacher-forced
     * passes always return log-probabilities (AttModel._forward). */
    int raw_logits;
} capmi_updown_rollout;

int64_t capmi_updown_planes_bytes(int R, int E);

int capmi_updown_rollout_fwd(const capmi_updown_weights *w, capmi_updown_rollout *r, void *stream);

typedef struct capmi_updown_grads {
    float *embed;
    float *att_w_ih, *att_w_hh, *att_b_ih, *att_b_hh;
    float *lang_w_ih, *lang_w_hh, *lang_b_ih, *lang_b_hh;
    float *h2att_w, *h2att_b;
    float *alpha_w, *alpha_b;
    float *logit_w, *logit_b;
    float *d_fc;       /* [B,R]   gradient w.r.t. prepared fc   */
    float *d_att;      /* [B,K,R] gradient w.r.t. prepared att (attention path only) */
    float *d_p_att;    /* [B,K,A] */
} capmi_updown_grads;

typedef struct capmi_updown_bwd_scratch {
    float *dlogits;     /* [T,N,V1]  time-major */
    float *d_hdrop;     /* [T,N,R]     */
    float *dg_att;      /* [T,N,4R]    */
    float *dg_lang;     /* [T,N,4R]    */
    float *d_x2;        /* [T,N,3R]  per step (d_ctx | dh_att | dh_lang_prev) = dg_lang [W_ih | W_hh] */
    float *d_e_all;     /* [T,N,K]     */
    float *d_att_h_all; /* [T,N,A]     */
    float *dh_att_attn; /* [N,R]       */
    float *d_x1;        /* [T,N,2R]  per step (dh_lang_prev | dh_att_prev) = dg_att [W_ih[:, :R] | W_hh] */
    float *dc_att, *dc_lang;   /* [2][N,R] ping-pong */
    float *d_xt_all;    /* [T,N,E]     */
    float *sum_dg_att;  /* [B,4R]      */
    float *w_lang_cat;  /* [4R,3R]  = [lang W_ih | lang W_hh], packed once per BPTT: one dX GEMM per step */
    float *w_att_cat;   /* [4R,2R]  = [att W_ih(:, 0:R) | att W_hh] */
    float *partial;
    int64_t partial_capacity;
    const capmi_sparse_logp_grad *sparse;   /* NULL, or the loss gradient in sparse form (then g_seq_logp may be NULL) */
    /* Rows [0, n_grad_rows) of the rollout carry gradient (0: all N).  The fused SCST rollout (row_img) keeps its greedy-baseline
     * rows behind the sampled ones; with n_grad_rows = B * n the backward runs on the sampled rows only and every [T,N,..]
     * array above is [T,n_grad_rows,..].  It then needs `pack`: >= n_grad_rows * (T * (4R + 2E + 2 + A + K) + R) + 64 floats
     * for gap-free copies of the saved activations. */
    int n_grad_rows;
    float *pack;
    int64_t pack_capacity;
    /* Round 3, optional (gradient rows <= 64): scratch for the A planes of d_gates of the two LSTM cells + a zero image
     * (capmi_updown_bwd_planes_bytes(R) bytes, zero-filled once by the caller); the dX GEMMs of the BPTT then stage their
     * activations by LDS-DMA.  NULL keeps the in-GEMM split. */
    void *planes;
    int64_t planes_bytes;
} capmi_updown_bwd_scratch;

int64_t capmi_updown_bwd_planes_bytes(int R);

/* g_seq_logp [N,T,V1]: gradient w.r.t. the dense log-probs returned by the forward (NULL when s->sparse carries it). */
int capmi_updown_rollout_bwd(const capmi_updown_weights *w, const capmi_updown_rollout *r,
                             const float *g_seq_logp, capmi_updown_bwd_scratch *s,
                             capmi_updown_grads *g, void *stream);

/* The same backward in separately callable phases, in this order, so that a data-parallel caller can start the
 * all-reduce of a gradient bucket while later phases still compute (phases is a bit mask; a full backward is
 * CAPMI_BWD_ALL or the five phases one after the other on the same stream):
 *   LOGIT      -> g->logit_w, logit_b (and d_hdrop for the recurrent part)
 *   RECURRENT  -> the BPTT loop (no parameter gradient yet)
 *   LANG_LSTM  -> g->lang_w_ih, lang_w_hh, lang_b_ih, lang_b_hh
 *   ATT_LSTM   -> g->att_w_ih, att_w_hh, att_b_ih, att_b_hh, embed, d_fc
 *   ATTENTION  -> g->h2att_w, h2att_b, alpha_w, alpha_b, d_att, d_p_att */
#define CAPMI_BWD_LOGIT 1
#define CAPMI_BWD_RECURRENT 2
#define CAPMI_BWD_LANG_LSTM 4
#define CAPMI_BWD_ATT_LSTM 8
#define CAPMI_BWD_ATTENTION 16
#define CAPMI_BWD_ALL 31
int capmi_updown_rollout_bwd_phases(const capmi_updown_weights *w, const capmi_updown_rollout *r,
                                    const float *g_seq_logp, capmi_updown_bwd_scratch *s,
                                    capmi_updown_grads *g, int phases, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched beam search for the UpDown decoder, entirely on the device (AttModel._sample_beam
 * AttModel.py:218-256 + CaptionModel.beam_search CaptionModel.py:35-209, group_size 1).
 * Replaces, per step: the full torch.sort over [B, b*V1] (:80) by a segmented top-b selection, the O(t)
 * re-gather of beam histories (:90-103) by parent pointers, the state gather (:105-109) by one reorder
 * kernel, and the 2*B*b `.item()` host syncs of the finished-beam loop (:183-198) by device flags.
 * ------------------------------------------------------------------------------------------- */
/* one selection step.  logp [B*cur, V1] (rows of image b: b*cur .. b*cur+cur-1), sums [B,cur] ->
 * top `bd` candidates per image sorted by descending score (ties: lowest flat index):
 * parent [B,bd] (beam the candidate extends), token [B,bd], score [B,bd] (= joint log-prob, recorded for
 * the finished-beam table), next_sums [B,bd] (= score, minus 1000 where the beam ended: token == 0 or
 * force_end), ended [B,bd]. */
int capmi_beam_select(const float *logp, const float *sums, int B, int cur, int bd, int V1, int force_end,
                      int32_t *parent, int64_t *token, float *score, float *next_sums, uint8_t *ended,
                      void *stream);
/* dst[a][b*bd + j][:] = src[a][b*cur + parent[b,j]][:] for `arrays` stacked [rows,R] arrays */
int capmi_beam_reorder(const float *src, float *dst, const int32_t *parent, int arrays, int B, int cur, int bd,
                       int R, void *stream);
/* out = log_softmax(log_softmax(logits) / temperature)  (CaptionModel.py:203-204 applies it to the already
 * normalised output); optionally out[:, unk_col] -= 1000 (suppress_UNK, :159-160; unk_col < 0: off). */
int capmi_beam_logsoftmax(const float *logits, float *out, int N, int V1, float temperature, int unk_col,
                          void *stream);

typedef struct capmi_updown_beam {
    int B, bd, K, A, R, E, V1, L;
    const float *fc, *att, *p_att, *att_mask;   /* prepared features of the B images */
    float temperature;
    int unk_col;            /* column to suppress by -1000, or -1 */
    /* work: state ping-pong [2][4][B*bd,R] (h_att,c_att,h_lang,c_lang), per-step scratch */
    float *state;
    float *xt, *gates, *att_h, *alpha, *ctx, *fc_gates, *logits;   /* [B*bd,*] scratch, fc_gates [B,4R] */
    int64_t *it;            /* [B*bd] */
    float *sums;            /* [2][B,bd] ping-pong */
    /* outputs, per step t */
    float *logp_rows;       /* [L][B*bd][V1]  normalised rows the selection of step t was made from
                               (step 0 uses only rows b*bd + 0) */
    int32_t *parent;        /* [L][B,bd] */
    int64_t *token;         /* [L][B,bd] */
    float *score;           /* [L][B,bd] */
    uint8_t *ended;         /* [L][B,bd] */
    float *partial; int64_t partial_capacity;
} capmi_updown_beam;

int capmi_updown_beam_search(const capmi_updown_weights *w, capmi_updown_beam *b, void *stream);

/* ONE UpDown decoder step on already prepared features: AttModel.get_logprobs_state (AttModel.py:166-176) up to the raw
 * logits (b->logits [rows,V1]); the caller normalises.  Tokens are read from b->it [rows]; `rows` = b->B *
 * rows_per_image hypotheses, image-major.  state_in / state_out are distinct [4][b->B*b->bd, R] arrays
 * (h_att, c_att, h_lang, c_lang).  first != 0 also (re)computes b->fc_gates.  Uses of b: B, bd (row capacity per image),
 * K, A, R, E, V1, fc, att, p_att, att_mask, xt, gates, att_h, alpha, ctx, fc_gates, logits, it, partial. */
int capmi_updown_decode_step(const capmi_updown_weights *w, capmi_updown_beam *b, int rows, int rows_per_image,
                             const float *state_in, float *state_out, int first, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Beam search as a TRAINING rollout ("SCST in Topdown Bottomup paper", reference ADVANCED.md; loss_wrapper.py with
 * train_sample_method greedy / train_beam_size > 1): search with the model's training numerics, finalise on the device, replay
 * the surviving beams through the forced rollout (capmi_updown_rollout_fwd / capmi_newfc_rollout_fwd) with the dropout masks
 * their ancestors saw.  A beam's log-probs are the decoder run along its own ancestry, so the replay's BPTT is the search's.
 * ------------------------------------------------------------------------------------------- */
/* capmi_updown_beam_search in train mode: `fc/att/p_att` of `b` are the DROPPED prepared features; the decoder call that
 * produces logp_rows[t] multiplies the word embedding of search row r by drop_xt[t][r][:] and the language LSTM output by
 * drop_out[t][r][:] (pre-scaled keep masks, [L][B*bd][E] and [L][B*bd][R]; call 0 runs on rows 0..B-1, one per image).
 * h_drop: [B*bd,R] scratch.  Either mask may be NULL (no dropout there). */
typedef struct capmi_updown_beam_train {
    capmi_updown_beam b;
    const float *drop_xt;
    const float *drop_out;
    float *h_drop;
} capmi_updown_beam_train;

int capmi_updown_beam_search_train(const capmi_updown_weights *w, capmi_updown_beam_train *bt, void *stream);

/* CaptionModel.py:183-208 on the device: from the [L][B,bd] tables of a finished search to the returned beams.  Per image
 * the candidates are the (t, j) with ended[t,b,j], in order of t then j; key p = (double)score / len_div[t] (len_div [L]
 * doubles on the device: the length penalty's divisor for a beam of t + 1 words, tabulated by the host so that the keys order
 * exactly as its own arithmetic does; NULL: p = score); stable descending sort; the best sample_n (1 <= sample_n <= bd) are
 * written to rows b*sample_n + i:
 *   seq [B*sample_n, L] int64 zero padded, length [B*sample_n] int32, p [B*sample_n] float,
 *   lineage [L][B*sample_n] int32: the search row (of logp_rows[t]) the beam's ancestor occupied at step t -- b at step 0
 *   (one row per image), b*bd + parent afterwards; -1 at and behind the beam's end.
 * One workgroup per image; L*bd <= 1024, bd <= 16.  The last step of a search ends every beam, so bd candidates always exist. */
int capmi_beam_finalize(const int32_t *parent, const int64_t *token, const float *score, const uint8_t *ended,
                        const double *len_div, int B, int bd, int L, int sample_n, int64_t *seq, int32_t *lineage,
                        int32_t *length, float *p, void *stream);

/* dst[t][i][:] = src[t][clamp(lineage[t][i], 0, rows_src - 1)][:] for up to two mask arrays in one launch (16-byte moves when
 * C_a, C_b % 4 == 0 and every pointer is 16-byte aligned, scalar moves otherwise; either pair may be NULL).
 * src [L][rows_src][C], dst [L][rows_dst][C], lineage [L][rows_dst]. */
int capmi_lineage_gather(const int32_t *lineage, int L, int rows_src, int rows_dst, const float *src_a, float *dst_a, int C_a,
                         const float *src_b, float *dst_b, int C_b, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Decode-time options (eval): the reference edits the [rows,V1] log-probabilities of a step on the host side
 * (AttModel.py:293-330, 391-432; CaptionModel.py:38-57, 152-157).  Here they are in-place device edits.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_DECODE_NO_REPEAT 1       /* decoding_constraint: the previous token gets -inf              */
#define CAPMI_DECODE_NO_BAD_ENDING 2   /* remove_bad_endings: column 0 gets -inf after a bad-ending word  */
#define CAPMI_DECODE_BLOCK_TRIGRAMS 4  /* block_trigrams: -0.693*2 per earlier occurrence of the trigram  */
/* logp [N,V1] in place.  prev[r*prev_stride] = token row r emitted at step t-1 (flags 1, 2; call only for t > 0).
 * bad_endings [n_bad] token ids.  seq [N,seq_ld] tokens emitted so far (columns 0..t-1; flag 4, rows < trigram_rows
 * only -- the reference loops over the image batch, AttModel.py:310, 322). */
int capmi_decode_constrain(float *logp, int N, int V1, const int64_t *prev, int prev_stride, int flags,
                           const int64_t *bad_endings, int n_bad, const int64_t *seq, int seq_ld, int t, int trigram_rows,
                           void *stream);
/* diverse beam search, CaptionModel.add_diversity (CaptionModel.py:38-57): out [B*cur,V1] = logp - change*lambda where
 * change[b,v] counts v among prev_tokens[b*prev_stride + 0..n_prev-1] (choices of the earlier groups at this local
 * time).  logp != out. */
int capmi_beam_diversity(const float *logp, float *out, int B, int cur, int V1, const int64_t *prev_tokens, int prev_stride,
                         int n_prev, float diversity_lambda, void *stream);
/* AttModel._diverse_sample (AttModel.py:395-397): logp[:, tokens] -= lambda for EVERY row, once per distinct token;
 * tokens[i*token_stride], i < n_tokens.  One call per earlier group. */
int capmi_column_penalty(float *logp, int N, int V1, const int64_t *tokens, int n_tokens, int token_stride,
                         float diversity_lambda, void *stream);

/* Logits processors (logits_proc.hip): hard n-gram blocking, repetition penalty, minimum length and banned word sequences, one
 * launch per decode step, one wave per row, in place on logp [rows] rows of V1 floats with pitch ld.  h = the row's history of t
 * tokens.  A row whose history holds the end token 0 is left untouched; the others get, in this order,
 *   repetition_penalty theta > 1   logp[v] = logp[v] * theta (one fp32 multiply) for every DISTINCT word v != 0 of h
 *   min_length m                   logp[0] = -inf while t < min(m, L - 1)
 *   no_repeat_ngram_size n >= 1    logp[v] = -inf for every v != 0 with h[i .. i+n-2] == h[t-n+1 .. t-1] and h[i+n-1] == v for
 *                                  some i <= t - n (n = 1: every word of h); words of exempt[img] are spared
 *   bad_words                      entry e of bad_len[e] = k ids bad_words[e * CAPMI_LP_BAD_LEN + 0 .. k-1] (all >= 1): its last
 *                                  id gets -inf when h ends with the k - 1 ids before it (k = 1: always) */
#define CAPMI_LP_HIST_MAX 64
#define CAPMI_LP_NGRAM_MAX 8
#define CAPMI_LP_BAD_MAX 16
#define CAPMI_LP_BAD_LEN 4
#define CAPMI_LP_BAD_IDS 64            /* CAPMI_LP_BAD_MAX * CAPMI_LP_BAD_LEN */
typedef struct {
    int no_repeat_ngram_size;          /* 0 = off, else 1 .. CAPMI_LP_NGRAM_MAX */
    float repetition_penalty;          /* 1 = off, else > 1 */
    int min_length;                    /* 0 = off */
    int n_bad;                         /* 0 .. CAPMI_LP_BAD_MAX */
    int bad_len[CAPMI_LP_BAD_MAX];
    int bad_words[CAPMI_LP_BAD_IDS];
} capmi_logits_proc;
/* The history is given in one of two forms.  Dense: seq [rows, seq_ld] int64, columns 0 .. t-1 (seq_ld >= t).  Back-pointer
 * (seq NULL): the per-step tables of a search, token int64 / parent int32 [L][rows / cur at step 0 = B][W]; at t > 0 the rows are
 * the W slots of step t - 1 (cur == W), row b * W + j has h[t-1] = token[t-1][b][j] and continues at slot parent[t-1][b][j] of step
 * t - 2; at t = 0 the history is empty.  cur: rows per image at this step (rows % cur == 0), img = row / cur.
 * exempt (or NULL) int32 [rows / cur][n_exempt]: per image, words the n-gram rule never blocks (entries < 1 are padding).
 * 0 <= t < L <= CAPMI_LP_HIST_MAX, else CAPMI_EINVAL; with every option off nothing is launched. */
int capmi_logits_process(float *logp, int ld, int rows, int V1, int t, int L, const capmi_logits_proc *p, const int64_t *seq,
                         int seq_ld, const int64_t *token, const int32_t *parent, int W, int cur, const int32_t *exempt,
                         int n_exempt, void *stream);
/* Token choice from rows that ALREADY hold (constrained) log-probabilities: nothing is renormalised, the rows are
 * stored as they are times the unfinished flag (AttModel.py:333-347; -inf * 0 = NaN like there).  mode 0 arg-max,
 * 1 Categorical(logits = logp / temperature) with the optional top-k / nucleus filter.  sel_logp [N,L] (optional):
 * the picked token's log-prob times the unfinished flag, or -- sel_unmasked != 0, AttModel._diverse_sample
 * (AttModel.py:436-447) -- sample_next_word's sampleLogprobs of the token the sampler picked, even for rows that had
 * finished: the row's entry (mode 0), the entry / temperature (mode 1, also under top-k), or under the nucleus filter
 * the log-prob of the renormalised truncated distribution (CaptionModel.py:396-398, 406).  Other arguments as in
 * capmi_logsoftmax_select_partial. */
int capmi_select_logp(const float *logp, int N, int V1, int step, int L, int mode, float temperature, const float *gumbel,
                      uint64_t seed, int64_t *seq, int seq_ld, int64_t *it_next, uint8_t *unfinished, float *seq_logp,
                      float *sel_logp, int sel_unmasked, const capmi_sample_filter *filter, void *stream);

/* Truncation samplers: min-p, epsilon and eta sampling (Hewitt et al. 2022), locally typical sampling (Meister et al. 2022).
 * x = row r of logp [N, ld] (already constrained log-probabilities, any per-row shift), p = softmax(x / temperature),
 * H = -sum p log p (0 log 0 = 0), p_max = max p.  The kept set of `kind` with parameter `param`:
 *   MINP (0 < a <= 1)   p_v >= a p_max
 *   EPS  (0 < e < 1)    p_v >= e, and every token with p_v == p_max
 *   ETA  (0 < e < 1)    p_v >= min(e, sqrt(e) exp(-H)), and every token with p_v == p_max
 *   TYP  (0 < tau < 1)  s_v <= s*, where s_v = |-log p_v - H| and s* is the smallest score with mass{v : s_v <= s*} >= tau
 *                       (tokens tied at s* are all kept)
 * Entries at -inf have p = 0 and are never kept; a row needs one finite entry.  q [N, ld_q], q != logp and no overlap:
 * q_v = log(p_v / sum_kept p) on the kept set, -inf elsewhere, so a draw of the rule is capmi_select_logp on q in mode 1 at
 * temperature 1 with no filter.  kept [N] (optional): the size of the kept set; kept_mass [N] (optional): sum_kept p.
 * store (optional): store[r * store_ld + v] = logp[r, v] * unfinished[r] (unfinished NULL: the row as it is; a finished row
 * holds x * 0, -inf * 0 = NaN, AttModel.py:345), the flag as it stands BEFORE this step's select -- what capmi_select_logp
 * writes through seq_logp.  Rows with V1 <= 12288 whose logp rows are all 16-byte aligned stay in registers across the passes;
 * any other row, and every row with CAPMI_TRUNCATE_STREAM OR-ed into `kind`, is re-read from memory per pass.  On the same row
 * (same alignment) the two arms give the same bits. */
#define CAPMI_TRUNCATE_MINP 0
#define CAPMI_TRUNCATE_EPS 1
#define CAPMI_TRUNCATE_ETA 2
#define CAPMI_TRUNCATE_TYP 3
#define CAPMI_TRUNCATE_STREAM 256
int capmi_truncate_rows(const float *logp, int ld, float *q, int ld_q, int N, int V1, int kind, float param, float temperature,
                        int *kept, float *kept_mass, float *store, int64_t store_ld, const uint8_t *unfinished, void *stream);

/* Contrastive search (Su et al. 2022), sample_method 'contrastive' (decode.contrastive_steps): at every step the k most probable
 * tokens of a row are re-scored by  (1 - alpha) p(v) - alpha max_s cos(g_v, h_s),  g_v the pre-logit row of the decoder after it
 * consumed candidate v and h_0 .. h_{len-1} the pre-logit rows the caption has produced so far (h_0: after BOS).
 *
 * capmi_contrastive_topk: tok [N, k] int64 / tok_logp [N, k] = the k largest entries of every row of logp [N, ld] in descending
 * order, equal values by ascending token id; -inf entries are values like any other, so a row with fewer than k finite entries is
 * filled with its lowest-numbered -inf columns.  1 <= k <= min(CAPMI_CONTRASTIVE_KMAX, V1).  store (optional):
 * store[r * store_ld + v] = logp[r, v] * unfinished[r], as capmi_truncate_rows has it.
 *
 * capmi_contrastive_select, ONE launch per generated token.  In: cand_tok / cand_logp [N, k] (the top-k output), cand_h [N * k, R]
 * with leading dimension ld (row i * k + j: candidate j of row i), hist [N, S_max, R] with hist_inv [N, S_max] = 1 / |h_s| (inf
 * for a zero row) of which the first hist_len rows are valid, the step t of L, alpha in [0, 1].
 *   score_j = (1 - alpha) exp(cand_logp_j) - alpha max_{s < hist_len} cos(g_j, h_s),   cos(a, b) = a.b / max(|a| |b|, 1e-8)
 * (torch.nn.functional.cosine_similarity's clamp: a zero row gives 0); cand_logp_j = -inf scores -inf; hist_len = 0: no penalty.
 * c = arg-max_j score_j, the lowest j on ties (all -inf: 0).  Out, each optional unless noted:
 *   choice [N] = c, parent [N] = i * k + c, fan [N, k] = c in every column (the parent table that reorders the decoder state of
 *   row i * k + c onto all k rows of image i, ready for the next look-ahead step);
 *   seq[i * seq_ld + t] = it[i] = cand_tok[i, c] where unfinished[i], else 0; unfinished[i] &= token != 0;
 *   hist[i, hist_len, :] = g_c and hist_inv[i, hist_len] = 1 / |g_c| (always written).
 * cand_tok NULL: no token outputs; cand_logp NULL: every p is 0 -- with k = 1 and hist_len = 0 the call that files the BOS row h_0.
 * Limits (CAPMI_EINVAL): 1 <= k <= CAPMI_CONTRASTIVE_KMAX, R >= 1 (no upper bound: rows are streamed), ld >= R, 0 <= t < L,
 * S_max >= L + 1, 0 <= hist_len < S_max, cand_h and hist apart.  |g|^2 is summed in double (the stored inverse norm is good to a float ulp), the dots in fp32, with 16-byte loads when R % 4 == 0,
 * ld % 4 == 0 and cand_h, hist sit on 16-byte boundaries, element by element otherwise. */
#define CAPMI_CONTRASTIVE_KMAX 32
int capmi_contrastive_topk(const float *logp, int ld, int N, int V1, int k, const uint8_t *unfinished, int64_t *tok,
                           float *tok_logp, float *store, int64_t store_ld, void *stream);
int capmi_contrastive_select(const int64_t *cand_tok, const float *cand_logp, const float *cand_h, int ld, float *hist,
                             float *hist_inv, int N, int k, int R, int S_max, int hist_len, int t, int L, float alpha,
                             int32_t *choice, int32_t *parent, int32_t *fan, int64_t *seq, int seq_ld, int64_t *it,
                             uint8_t *unfinished, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Transformer captioner building blocks (BASELINE configs[3]; TransformerModel.py).  The contractions
 * (QKV / output projections, FFN, generator) run on capmi_gemm_f32 with fused bias / ReLU / dropout /
 * residual epilogues; these are the non-GEMM pieces.
 * ------------------------------------------------------------------------------------------- */
/* custom LayerNorm of the reference (TransformerModel.py:76-87): y = a*(x-mean)/(std_unbiased+eps)+b.
 * x,y [M,D]; saves mean[M] and inv[M] = 1/(std+eps) for the backward. */
int capmi_layernorm_fwd(const float *x, const float *a, const float *b, float *y, float *mean, float *inv,
                        int M, int D, float eps, void *stream);
/* dx [M,D] (accumulate: dx += ... for the residual branch), g_scaled [M,D] = dy*(x-mean)*inv (column-sum it
 * for d_a; column-sum dy for d_b). */
int capmi_layernorm_bwd(const float *dy, const float *x, const float *a, const float *mean, const float *inv,
                        float *dx, int accumulate, float *g_scaled, int M, int D, float eps, void *stream);
/* r6: the same backward with the PARAMETER gradients started in the launch: every workgroup leaves the sums of dy (x - mean) inv and of
 * dy over its own rows (fixed order) as one row of part_a / part_b, [capmi_layernorm_bwd_parts_rows(M), D] each; d_a / d_b are their
 * column sums (capmi_colsum_batch over ~M/8 rows instead of M, and no [M, D] g_scaled is written).  Deterministic.  D <= 2048. */
int capmi_layernorm_bwd_parts_rows(int M);
int capmi_layernorm_bwd_parts(const float *dy, const float *x, const float *a, const float *mean, const float *inv, float *dx,
                              int accumulate, float *part_a, float *part_b, int M, int D, float eps, void *stream);
/* r5, AoA decode step (AoAModel.py:163-186): the same backward when BOTH inputs are still K-slice slabs of the GEMMs that made
 * them -- dy = sum_s dy_slabs[s] ([M,D] slabs dy_stride floats apart; the finished dy is also written to dy_out when not NULL: its
 * column sums are d_b) and the running gradient the LayerNorm term is added to, dx = sum_s acc_slabs[s] + ..., slabs of row pitch
 * acc_ld (a column block of a wider product: the query half of d_cat, AoAModel.py:174) acc_stride floats apart.  Slabs are added
 * in slab order from 0.f, the bits of capmi_splitk_reduce / capmi_split_halves followed by capmi_layernorm_bwd(accumulate=1). */
int capmi_layernorm_bwd_slabs(const float *dy_slabs, int dy_splits, int64_t dy_stride, float *dy_out, const float *x, const float *a,
                              const float *mean, const float *inv, const float *acc_slabs, int acc_splits, int64_t acc_stride,
                              int acc_ld, float *dx, float *g_scaled, int M, int D, float eps, void *stream);
/* multi-head scaled-dot-product attention for short sequences (TransformerModel.py:152-195), one workgroup
 * per (key/value batch row, head).  q [Nq,Tq,D], k,v rows of pitch ldkv floats ([Nkv,Tk,D] or a KV cache
 * [Nkv,Lmax,D]), D = h*dk, heads interleaved along D exactly like `.view(N,-1,h,dk)`.  Query row r attends
 * key/value batch row r / q_per_kv (cross-attention over per-image memory: no repeat_tensors copy).
 * kstride: floats between consecutive keys of one kv row (D for packed [Tk,D]; 2R when K and V are the two halves of
 * AoA's p_att rows, AoAModel.py:168).  mask: uint8 [Nq or Nkv-broadcast, mask_tq (1 or Tq), Tk] (0 = -inf), or NULL; causal != 0 additionally
 * masks key j > query position (q_pos0 + i).  drop: optional pre-scaled keep mask [Nq,h,Tq,Tk] applied to the
 * probabilities.  Outputs o [Nq,Tq,D] and p [Nq,h,Tq,Tk] (softmax probabilities BEFORE dropout, saved).
 * dk % 4 == 0 and 16-byte aligned q / k / v / o rows (ldkv, kstride multiples of 4): the head dimension moves in 16-byte pieces. */
int capmi_mha_fwd(const float *q, const float *k, const float *v, int ldkv, int kstride, const uint8_t *mask, int mask_tq,
                  int mask_per_q, int causal, int q_pos0, const float *drop, float *o, float *p, int Nq, int q_per_kv,
                  int Tq, int Tk, int h, int dk, void *stream);
/* Same with a query row pitch: qstride floats between consecutive query rows (0 = D).  Lets q, k, v be the three column blocks
 * of ONE fused projection y = x [Wq; Wk; Wv]^T of pitch 3D (r4: the three Linear calls of TransformerModel.py:179-181 as one
 * GEMM with N = 3D; k, v then use kstride = 3D). */
int capmi_mha_fwd_s(const float *q, int qstride, const float *k, const float *v, int ldkv, int kstride, const uint8_t *mask,
                    int mask_tq, int mask_per_q, int causal, int q_pos0, const float *drop, float *o, float *p, int Nq,
                    int q_per_kv, int Tq, int Tk, int h, int dk, void *stream);
/* r5: q still as the K-slice slabs of its projection GEMM (q_splits >= 1 slabs of row pitch qstride, q_slab_stride floats apart):
 * every workgroup finishes its head's columns -- slabs in order from 0.f, + q_bias (NULL = none): the bits of capmi_splitk_reduce --
 * and writes them to q_out [Nq,Tq,D] (NULL = not wanted) for the backward.  q_splits = 0: plain capmi_mha_fwd_s. */
int capmi_mha_fwd_qslabs(const float *q, int qstride, int q_splits, int64_t q_slab_stride, const float *q_bias, float *q_out,
                         const float *k, const float *v, int ldkv, int kstride, const uint8_t *mask, int mask_tq, int mask_per_q,
                         int causal, int q_pos0, const float *drop, float *o, float *p, int Nq, int q_per_kv, int Tq, int Tk, int h,
                         int dk, void *stream);
/* backward: d_o [Nq,Tq,D] -> dq [Nq,Tq,D], dk/dv summed over the q_per_kv query rows of a kv row, written at
 * out + kv_row*dkv_ld + key*dkv_stride (+= when accumulate: BPTT over time steps) */
int capmi_mha_bwd(const float *d_o, const float *q, const float *k, const float *v, int ldkv, int kstride, const float *p,
                  const float *drop, float *dq, float *dk_out, float *dv_out, int dkv_ld, int dkv_stride, int accumulate,
                  int Nq, int q_per_kv, int Tq, int Tk, int h, int dk, void *stream);
/* Same with query / dq row pitches (0 = D): dq may be a column block of the fused [rows, 3D] gradient that one dX GEMM
 * (K = 3D) and one dW GEMM consume. */
int capmi_mha_bwd_s(const float *d_o, const float *q, int qstride, const float *k, const float *v, int ldkv, int kstride,
                    const float *p, const float *drop, float *dq, int dq_stride, float *dk_out, float *dv_out, int dkv_ld,
                    int dkv_stride, int accumulate, int Nq, int q_per_kv, int Tq, int Tk, int h, int dk, void *stream);
/* r5: d_o with a row pitch do_ld >= D and possibly still `do_splits` K-slice slabs do_stride floats apart (the attention half of
 * d_cat in an AoA decode step), summed in slab order from 0.f like capmi_split_halves.  do_splits = 1, do_ld = D: capmi_mha_bwd_s. */
int capmi_mha_bwd_slabs(const float *d_o, int do_splits, int64_t do_stride, int do_ld, const float *q, int qstride, const float *k,
                        const float *v, int ldkv, int kstride, const float *p, const float *drop, float *dq, int dq_stride,
                        float *dk_out, float *dv_out, int dkv_ld, int dkv_stride, int accumulate, int Nq, int q_per_kv, int Tq,
                        int Tk, int h, int dk, void *stream);
/* Host only, launches nothing: the launch shape the forward (bwd = 0) or backward (bwd = 1) entry points above choose for these
 * sizes -- CH query rows per LDS pass, threads per workgroup, mfma (1: contractions on the matrix pipe), lds bytes of dynamic
 * LDS.  Returns CAPMI_EINVAL where the launchers refuse the sizes (more than 160 KB of LDS, dk % 4, Nq % q_per_kv). */
int capmi_mha_plan(int bwd, int Nq, int q_per_kv, int Tq, int Tk, int h, int dk, int *CH, int *threads, int *mfma, int64_t *lds);
/* x[r,t,:] = E[tok[r,t]]*sqrt(D) + pe[pos0+t,:], then * drop (TransformerModel.py:215, 231-233) */
int capmi_embed_pe_fwd(const int64_t *tok, int tok_ld, const float *E, const float *pe, const float *drop, float *x,
                       int N, int T, int D, int pos0, void *stream);
/* dE[tok] += dx*drop*sqrt(D)  (caller zeroes dE) */
int capmi_embed_pe_bwd(const int64_t *tok, int tok_ld, const float *dx, const float *drop, float *dE, int N, int T, int D,
                       void *stream);
/* AoA / GLU blocks (AoAModel.py:44, 143): out = [residual +] mask * (pre[:, :R] * sigmoid(pre[:, R:2R])), pre [M,2R] */
int capmi_glu_fwd(const float *pre, const float *mask, const float *residual, float *out, int M, int R, void *stream);
/* The same for one AoA decode step, finishing the att2ctx GEMM's K-slice slabs itself (slabs [splits][M,2R] + bias -> pre, kept
 * for the backward) and writing every consumer's operand: out, out_a = out * mask_a (input of the logit GEMM), out_b = out * mask_b
 * (context input of the NEXT step) -- masks NULL = plain copies, out_a / out_b NULL = not wanted -- the last two also as "A planes"
 * (M <= 64; capmi_planes_from_f32 layout, buffers zero-filled once by the caller).  R % 4 == 0, 16-byte aligned operands. */
int capmi_glu_fwd_fused(const float *slabs, int splits, int64_t stride, const float *bias, float *pre, float *out,
                        const float *mask_a, float *out_a, void *planes_a, const float *mask_b, float *out_b, void *planes_b,
                        int M, int R, void *stream);
/* The att2ctx stage of one AoA decode step for every decoder_type (AoAModel.py:141-149, 172-185): siblings of
 * capmi_glu_fwd_fused that read the same slab layout (slabs [splits][M, G*R], `stride` floats apart, summed in order from 0.f,
 * then bias + bias2) and write the same outputs and planes.
 *   CAPMI_CTX_GLU  (G = 2)  out = a * sigmoid(g), pre [M,2R] kept for capmi_glu_bwd_add
 *   CAPMI_CTX_RELU (G = 1)  out = max(pre, 0); the backward takes its mask from `out` (capmi_relu_bwd_add), pre is not written
 *   CAPMI_CTX_LSTM (G = 4)  an nn.LSTMCell over the gate slabs of [att, h_att] W_ih + h_logic W_hh: bias = b_ih, bias2 = b_hh,
 *                           c = f * c_prev + i * g, out = o * tanh(c); pre (may be NULL) receives the ACTIVATED gates [M,4R] in the
 *                           layout capmi_lstm_cell_bwd_partial reads
 * out_a = mask_a * (out + resid): the logit GEMM's input; resid (NULL = none) is h_att under out_res, added before the dropout.
 * out_b = mask_b * out: the context input of the NEXT step (never with the residual).  A NULL mask is a plain copy -- the mask
 * is not read, nothing is multiplied (ctx_drop 0).  out_a / out_b NULL = not wanted; planes as in capmi_glu_fwd_fused (M <= 64).
 * R % 4 == 0, 16-byte aligned operands. */
#define CAPMI_CTX_GLU 0
#define CAPMI_CTX_RELU 1
#define CAPMI_CTX_LSTM 2
typedef struct {
    const float *slabs;
    const float *bias, *bias2;
    float *pre;
    const float *c_prev;
    float *c;
    float *out;
    const float *resid;
    const float *mask_a;
    float *out_a;
    void *planes_a;
    const float *mask_b;
    float *out_b;
    void *planes_b;
    int64_t stride;
    int kind, splits, M, R;
} capmi_ctx_step;
int capmi_ctx_fwd_fused(const capmi_ctx_step *s, void *stream);
/* d_pre [M,R] = (out > 0) * (d_out + add_mask * sum_s add_slabs[s]): the backward of CAPMI_CTX_RELU with the second gradient
 * source of capmi_glu_bwd_add (same order of additions); `out` is the saved forward output. */
int capmi_relu_bwd_add(const float *d_out, const float *add_slabs, int add_splits, int64_t add_stride, const float *add_mask,
                       const float *out, float *d_pre, int M, int R, void *stream);
/* d_pre [M,2R] from d_out [M,R] (mask applied first) */
int capmi_glu_bwd(const float *d_out, const float *mask, const float *pre, float *d_pre, int M, int R, void *stream);
/* r5: the same with a second gradient source that is still K-slice slabs: g = mask * d_out + add_mask * sum_s add_slabs[s]
 * ([M,R] slabs add_stride floats apart, added in slab order from 0.f, then the mask, then the sum: the bits of a split-K reduction
 * with mul_mask + accumulate into d_out).  In an AoA BPTT step it is the gradient reaching out_t through step t+1's context input
 * (AoAModel.py:165-166), whose GEMM then needs no reduce launch. */
int capmi_glu_bwd_add(const float *d_out, const float *mask, const float *add_slabs, int add_splits, int64_t add_stride,
                      const float *add_mask, const float *pre, float *d_pre, int M, int R, void *stream);
/* out_lo [M,R] = mask_lo * sum_s slabs[s][:, 0:R], out_hi [M,R] = mask_hi * sum_s slabs[s][:, R:2R]: the two halves of a [M,2R]
 * product that is still `splits` K-slice slabs of pitch `stride` floats (or a finished matrix, splits = 1), each through its
 * dropout mask (NULL = none).  The backward of torch.cat([att, query], -1) in the AoA blocks (AoAModel.py:92,174): d_cat = d_pre W
 * feeds two consumers that want contiguous [M,R] operands -- one launch instead of a split-K reduction, two slice copies and
 * two mask multiplies. */
int capmi_split_halves(const float *slabs, int splits, int64_t stride, const float *mask_lo, const float *mask_hi, float *out_lo,
                       float *out_hi, int M, int R, void *stream);
/* masked mean over regions (AoAModel.py:214-219): mean[b,:] = sum_k m[b,k] x[b,k,:] / sum_k m[b,k] (m NULL = ones) */
int capmi_meanpool_fwd(const float *x, const float *mask, float *mean, int B, int K, int D, void *stream);
/* dx[b,k,:] (+)= m[b,k]/cnt * dmean[b,:] */
int capmi_meanpool_bwd(const float *dmean, const float *mask, float *dx, int accumulate, int B, int K, int D, void *stream);
/* r6: caption statistics of the evaluation loop (captioning/utils/eval_utils.py:173-174) from a decode's dense log-probs
 * seq_logp [N, L, V1] and tokens seq [N, L]:
 *   entropy[r]    = -sum_t sum_v softmax(seq_logp[r,t,:])_v * seq_logp[r,t,v] / (count(seq[r,:] > 0) + 1)
 *   perplexity[r] = -sum_t seq_logp[r,t,seq[r,t]]                            / (count(seq[r,:] > 0) + 1)
 * One pass over seq_logp, no dense temporaries (the ATen formula built three).  A -inf log-prob contributes 0 (0 * -inf := 0).
 * scratch: 2 * N * L floats.  V1 <= 32768. */
int capmi_caption_stats(const float *seq_logp, const int64_t *seq, int N, int L, int V1, float *scratch, float *entropy, float *perplexity,
                        void *stream);
/* out = log_softmax(logits) row-wise (Generator, TransformerModel.py:50-57) */
int capmi_log_softmax_rows(const float *logits, float *out, int rows, int V1, void *stream);

/* ---------------------------------------------------------------------------------------------
 * NewFC decoder (BASELINE configs[0], configs/fc.yml): NewFCModel (AttModel.py:904-945) over the maxout
 * LSTMCore (FCModel.py:13-42).  The image embedding is fed as a first LSTM step when the state is all
 * zero (AttModel.py:925-927), then one word per step; log-softmax / choice / bookkeeping are shared
 * with the UpDown path (capmi_logsoftmax_select).
 * ------------------------------------------------------------------------------------------- */
/* maxout cell: sums = sum_s partial[s] + b_i2h + b_h2h ([N,5R]: in, forget, out, cand_a, cand_b);
 * c' = sig(f)*c + sig(in)*max(cand_a,cand_b); h' = sig(out)*tanh(c').  saved [N,5R] = (sig(in), sig(f),
 * sig(out), cand_a, cand_b). */
int capmi_maxout_cell_fwd(const float *partial, int splits, const float *b_i2h, const float *b_h2h,
                          const float *c_prev, float *h, float *c, float *saved, const float *out_mask,
                          float *h_drop, int N, int R, void *stream);
/* dh = dh_a (* dh_a_mask) + dh_b; d_sums [N,5R]; dc_prev [N,R] */
int capmi_maxout_cell_bwd(const float *dh_a, const float *dh_a_mask, const float *dh_b, const float *dc_next,
                          const float *saved, const float *c_prev, const float *c_new, float *d_sums,
                          float *dc_prev, int N, int R, void *stream);

typedef struct capmi_newfc_weights {
    const float *embed;            /* [V1,E]  embed.weight (plain Embedding, AttModel.py:908) */
    const float *i2h_w, *i2h_b;    /* [5R,E],[5R]  _core.i2h */
    const float *h2h_w, *h2h_b;    /* [5R,R],[5R]  _core.h2h */
    const float *logit_w, *logit_b;
} capmi_newfc_weights;

typedef struct capmi_newfc_rollout {
    int B, n, N, R, E, V1, T, L;
    const float *fc_emb;    /* [B,E]  fc_embed(fc_feats) (no ReLU / dropout: AttModel.py:907) */
    const float *drop_out;  /* [T,N,R] keep masks for the LSTMCore output dropout, or NULL */
    int mode; float temperature; const float *gumbel; uint64_t seed;
    const int64_t *forced; int forced_ld; int teacher;
    float *h, *c;           /* [T+2,N,R]  slot 0 zeros, slot 1 after the image step, slot t+2 after word t */
    float *x;               /* [T,N,E]   word embeddings */
    int64_t *it_all;        /* [T,N] */
    float *saved;           /* [T+1,N,5R] cell activations, slot 0 = image step */
    float *h_drop;          /* [T,N,R] */
    int64_t *seq; float *seq_logp; float *sel_logp; uint8_t *live;   /* [N,L], [N,L,V1], [N,L], [N,L] */
    float *logits; int64_t *it; uint8_t *unfinished;
    float *partial; int64_t partial_capacity;
    /* scheduled sampling (teacher == 1 only, else CAPMI_EINVAL; AttModel.py:145-154): [T,N] or NULL, same meaning as
     * capmi_updown_rollout.ss_mode.  ss_mode[t*N + r] says where the INPUT token of row r at step t comes from: 2 = forced[r, t],
     * 1 = a draw (Gumbel-max, temperature 1, `seed` / `gumbel`) from the model's own distribution of step t-1.  Row t = 0 is not
     * read: the first input is always forced[:, 0].  The select launch of step t < T-1 chooses and embeds the input of step t+1
     * (x[t+1], it_all[t+1]), so such a step has no embedding launch.  Last field: older callers' layout is unchanged. */
    const uint8_t *ss_mode;
} capmi_newfc_rollout;

typedef struct capmi_newfc_grads {
    float *embed, *i2h_w, *i2h_b, *h2h_w, *h2h_b, *logit_w, *logit_b;
    float *d_fc_emb;   /* [B,E] */
} capmi_newfc_grads;

typedef struct capmi_newfc_bwd_scratch {
    float *dlogits;   /* [T,N,V1] */
    float *d_hdrop;   /* [T,N,R]  */
    float *d_sums;    /* [T+1,N,5R] slot 0 = image step */
    float *dh_prev;   /* [2][N,R] ping-pong */
    float *dc;        /* [2][N,R] */
    float *d_x_all;   /* [T,N,E]  */
    float *d_ximg;    /* [N,E]    */
    float *partial; int64_t partial_capacity;
    const capmi_sparse_logp_grad *sparse;   /* as in capmi_updown_bwd_scratch */
} capmi_newfc_bwd_scratch;

int capmi_newfc_rollout_fwd(const capmi_newfc_weights *w, capmi_newfc_rollout *r, void *stream);
int capmi_newfc_rollout_bwd(const capmi_newfc_weights *w, const capmi_newfc_rollout *r, const float *g_seq_logp,
                            capmi_newfc_bwd_scratch *s, capmi_newfc_grads *g, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Att2in2 decoder (configs/a2i2*.yml): Att2in2Model (AttModel.py:854-859) over Att2in2Core (:750-790).
 * Per step: att_res = Attention(h_prev) (the capmi_attention_* kernels, queried with the state BEFORE the
 * step); sums = i2h(x) + h2h(h_prev) [N,5R]; the candidate half (columns 3R..5R) also gets a2c(att_res);
 * then the maxout cell of NewFC.  Embedding = ReLU + dropout (AttModel.py:74-76), BOS first, no image step.
 * ------------------------------------------------------------------------------------------- */
/* cell: sums = sum_s partial[s] (+ addend) + b_i2h + b_h2h ([N,5R] slabs, stride N*5R), and on columns 3R..5R also
 * sum_s partial2[s] + b_a2c ([N,2R] slabs of the a2c GEMM, stride N*2R; splits2 = 0: none).  Outputs as
 * capmi_maxout_cell_fwd: h, c, saved [N,5R] = (sig(in), sig(f), sig(out), cand_a, cand_b), h_drop = h * out_mask. */
int capmi_att2in2_cell_fwd(const float *partial, int splits, const float *partial2, int splits2, const float *addend,
                           const float *b_i2h, const float *b_h2h, const float *b_a2c, const float *c_prev, float *h,
                           float *c, float *saved, const float *out_mask, float *h_drop, int N, int R, void *stream);
/* dh = dh_a (* dh_a_mask) + sum_{s<b_splits} dh_b[s*b_stride + r*R + j] (a dX GEMM left as slabs; NULL: none);
 * writes d_sums [N,5R] (whose columns 3R..5R are also the gradient of the a2c output) and dc_prev [N,R]. */
int capmi_att2in2_cell_bwd(const float *dh_a, const float *dh_a_mask, const float *dh_b, int b_splits, int64_t b_stride,
                           const float *dc_next, const float *saved, const float *c_prev, const float *c_new, float *d_sums,
                           float *dc_prev, int N, int R, void *stream);

typedef struct capmi_att2in2_weights {
    const float *embed;                /* [V1,E]  embed.0.weight */
    const float *i2h_w, *i2h_b;        /* [5R,E],[5R]  core.i2h */
    const float *h2h_w, *h2h_b;        /* [5R,R],[5R]  core.h2h */
    const float *a2c_w, *a2c_b;        /* [2R,R],[2R]  core.a2c */
    const float *h2att_w, *h2att_b;    /* [A,R],[A]    core.attention.h2att */
    const float *alpha_w, *alpha_b;    /* [A],[1]      core.attention.alpha_net */
    const float *logit_w, *logit_b;    /* [V1,R],[V1]  logit */
} capmi_att2in2_weights;

typedef struct capmi_att2in2_rollout {
    int B, n, N, K, A, R, E, V1, T, L;
    const float *att, *p_att, *att_mask;   /* [B,K,R] att_embed output, [B,K,A] ctx2att output, [B,K] or NULL */
    const float *drop_xt, *drop_out;       /* [T,N,E], [T,N,R] keep masks (embedding / core output dropout) or NULL */
    int mode; float temperature; const float *gumbel; uint64_t seed;
    const int64_t *forced; int forced_ld; int teacher;
    const uint8_t *ss_mode;   /* [T,N] or NULL (teacher only): scheduled sampling, as capmi_updown_rollout.ss_mode */
    float *h, *c;             /* [T+1,N,R]  slot 0 = zero state, slot t+1 after step t */
    float *x;                 /* [T,N,E]    input embeddings */
    int64_t *it_all;          /* [T,N]      input tokens */
    float *xin;               /* [T,N,5R]   teacher forcing: i2h product of all steps (one GEMM), or NULL */
    float *att_h, *alpha, *ctx;   /* [T,N,A], [T,N,K], [T,N,R] */
    float *saved, *h_drop;    /* [T,N,5R], [T,N,R] */
    int64_t *seq; float *seq_logp; float *sel_logp; uint8_t *live;   /* [N,L], [N,L,V1], [N,L], [N,L] */
    int64_t *it; uint8_t *unfinished;
    float *partial; int64_t partial_capacity;
} capmi_att2in2_rollout;

typedef struct capmi_att2in2_grads {
    float *embed, *i2h_w, *i2h_b, *h2h_w, *h2h_b, *a2c_w, *a2c_b, *h2att_w, *h2att_b, *alpha_w, *alpha_b, *logit_w, *logit_b;
    float *d_att, *d_p_att;   /* [B,K,R], [B,K,A]: for the prefill backward (att_embed, ctx2att) */
} capmi_att2in2_grads;

typedef struct capmi_att2in2_bwd_scratch {
    float *dlogits;   /* [T,N,V1] */
    float *d_hdrop;   /* [T,N,R]  */
    float *d_sums;    /* [T,N,5R] */
    float *d_ctx;     /* [T,N,R]  */
    float *d_att_h;   /* [T,N,A]  */
    float *d_e;       /* [T,N,K]  */
    float *dc;        /* [2][N,R] */
    float *d_x;       /* [T,N,E]  */
    float *partial; int64_t partial_capacity;
    const capmi_sparse_logp_grad *sparse;   /* as in capmi_updown_bwd_scratch */
} capmi_att2in2_bwd_scratch;

int capmi_att2in2_rollout_fwd(const capmi_att2in2_weights *w, capmi_att2in2_rollout *r, void *stream);
int capmi_att2in2_rollout_bwd(const capmi_att2in2_weights *w, const capmi_att2in2_rollout *r, const float *g_seq_logp,
                              capmi_att2in2_bwd_scratch *s, capmi_att2in2_grads *g, void *stream);

/* one decode step in eval numerics (AttModel.get_logprobs_state up to the logits) for the host-stepped samplers:
 * rows = B * rows_per_image image-major rows, state (h, c) read from *_src and written to *_dst ([rows,R] each). */
typedef struct capmi_att2in2_step {
    int B, K, A, R, E, V1;
    const float *att, *p_att, *att_mask;   /* [B,K,R], [B,K,A], [B,K] or NULL */
    const int64_t *it;                      /* [rows] input tokens */
    float *xt, *att_h, *alpha, *ctx, *saved, *logits;   /* [rows, E | A | K | R | 5R | V1] */
    float *partial; int64_t partial_capacity;
} capmi_att2in2_step;
int capmi_att2in2_decode_step(const capmi_att2in2_weights *w, capmi_att2in2_step *s, int rows, int rows_per_image,
                              const float *h_src, const float *c_src, float *h_dst, float *c_dst, void *stream);

/* ---------------------------------------------------------------------------------------------
 * AdaAtt decoder (caption_model adaatt / adaattmo): AdaAttModel / AdaAttMOModel (AttModel.py:843-852) over AdaAttCore
 * (:604-613) = AdaAtt_lstm (:451-537, one layer) + AdaAtt_attention (:539-602).  Requires E == R == A (the views at
 * :569-582).  G = 4R (adaatt, tanh candidate) or 5R (adaattmo, maxout of the last two R-blocks).  Per step:
 *   sums [N, G+R] = (w2h | r_w2h)(x) + (h2h | r_h2h)(h_prev) + fc_gates[image]       fc_gates = (v2h | r_v2h)(fc) + all six biases
 *   cell: c, h, sentinel fake = sigmoid(sums[:, G:]) * tanh(c); h_drop = h * drop_h (the STATE keeps h), fake_drop = fake * drop_fake
 *   fr = relu(fr_linear(fake_drop)) * drop_fr;  ho = tanh(ho_linear(h_drop)) * drop_ho;  fr_e = fr_embed(fr);  ho_e = ho_embed(ho)
 *   sentinel attention over [fr_e ; p_att] / [fr ; att] queried with ho_e (+ ho);  out = tanh(att2h(.)) * drop_out -> logit.
 * ------------------------------------------------------------------------------------------- */
/* dropout of the [rows, K+1, A] tanh tile of the sentinel attention (AttModel.py:585).  mask: pre-scaled keep mask of the
 * launch's rows, or NULL with p > 0: keep = Philox4x32-10(seed)(element (row0 + row, score row, column)) >= p, value 1 / (1 - p);
 * the backward entry points regenerate the same bits from the same (seed, row0).  NULL struct / NULL mask and p == 0: none. */
typedef struct capmi_tile_drop {
    const float *mask;
    float p;
    uint64_t seed;
    int64_t row0;
} capmi_tile_drop;
/* AdaAtt_attention.forward (AttModel.py:579-598) for N = B * n image-major rows.  fre / hoe: fr_e / ho_e [N,A], finished
 * (splits == 0) or as the K-slice slabs of their GEMMs (stride in floats) to which the bias is added here; fre_out / hoe_out
 * (optional) receive the finished rows.  fr, ho [N,R]; p_att [B,K,A], att [B,K,R] are read once per workgroup; mask [B,K] or NULL:
 * the sentinel takes the mask of region 0 (:592).  pi [N,K+1] (sentinel first), ctx [N,R] = pi . [fr ; att] + ho (:598). */
int capmi_sentinel_attention_fwd(const float *fre, int fre_splits, int64_t fre_stride, const float *fre_bias, const float *hoe,
                                 int hoe_splits, int64_t hoe_stride, const float *hoe_bias, float *fre_out, float *hoe_out,
                                 const float *fr, const float *ho, const float *p_att, const float *att, const float *mask,
                                 const float *w, const float *b, const capmi_tile_drop *drop, float *pi, float *ctx, int B,
                                 int n, int K, int A, int R, void *stream);
/* its backward for the rows of T steps at once ([T,N,.] buffers; the attention output of a step feeds only that step's logits):
 * d_e [T,N,K+1], d_hoe [T,N,A] (the query gradient), d_fre [T,N,A], d_fr [T,N,R] = pi[:, 0] d_ctx.  The residual's gradient
 * (d_ho += d_ctx) is the caller's.  drop: the forward's, with mask covering [T,N,K+1,A] and row0 = 0. */
int capmi_sentinel_attention_bwd(const float *d_ctx, const float *fr, const float *fre, const float *hoe, const float *pi,
                                 const float *p_att, const float *att, const float *w, const capmi_tile_drop *drop, float *d_e,
                                 float *d_hoe, float *d_fre, float *d_fr, int T, int B, int n, int K, int A, int R,
                                 void *stream);
/* time-batched d_att [B,K,R], d_p_att [B,K,A], alpha_net gradients (d_w [A] by atomics, or dw_partial [B*(K+1), A] rows for the
 * caller to column-sum; d_b [1]) as capmi_attention_bwd_batched_ws. */
int capmi_sentinel_attention_bwd_batched(const float *d_ctx, const float *fre, const float *hoe, const float *pi,
                                         const float *d_e, const float *p_att, const float *w, const capmi_tile_drop *drop,
                                         float *d_att, float *d_p_att, float *d_w, float *d_b, int T, int B, int n, int K,
                                         int A, int R, float *dw_partial, void *stream);
/* AdaAtt_lstm.forward (AttModel.py:498-533), one launch: sums = sum_s partial[s] ([N,G+R] slabs) (+ addend [N,G+R])
 * + fc_gates[row / n]; saved [N,G+R] = (sig(in), sig(f), sig(out), candidate (tanh value | the two maxout inputs), sig(sentinel)). */
int capmi_adaatt_cell_fwd(const float *partial, int splits, const float *addend, const float *fc_gates, int n,
                          const float *c_prev, float *h, float *c, float *saved, const float *drop_h, const float *drop_fake,
                          float *h_drop, float *fake_drop, int N, int R, int maxout, void *stream);
/* dh = dh_a (* dh_a_mask) + sum_s dh_b[s * b_stride + i]; dfake = d_fake (* d_fake_mask); writes d_sums [N,G+R], dc_prev. */
int capmi_adaatt_cell_bwd(const float *dh_a, const float *dh_a_mask, const float *d_fake, const float *d_fake_mask,
                          const float *dh_b, int b_splits, int64_t b_stride, const float *dc_next, const float *saved,
                          const float *c_prev, const float *c_new, float *d_sums, float *dc_prev, int N, int R, int maxout,
                          void *stream);

typedef struct capmi_adaatt_weights {
    const float *embed;                      /* [V1,E]  embed.0.weight */
    const float *xw, *hw;                    /* [G+R,E], [G+R,R]: core.lstm (w2h | r_w2h) and (h2h.0 | r_h2h) weights stacked by rows */
    const float *fr_w, *fr_b, *ho_w, *ho_b;          /* [E,R],[E]  core.attention.fr_linear.0 / ho_linear.0 */
    const float *fre_w, *fre_b, *hoe_w, *hoe_b;      /* [A,E],[A]  core.attention.fr_embed / ho_embed */
    const float *alpha_w, *alpha_b;          /* [A],[1]    core.attention.alpha_net */
    const float *att2h_w, *att2h_b;          /* [R,R],[R]  core.attention.att2h */
    const float *logit_w, *logit_b;          /* [V1,R],[V1] logit */
} capmi_adaatt_weights;

typedef struct capmi_adaatt_rollout {
    int B, n, N, K, A, R, E, V1, T, L, maxout;
    const float *fc_gates;                   /* [B,G+R] (v2h | r_v2h)(fc_embed(fc)) + the six gate biases: one product per rollout */
    const float *att, *p_att, *att_mask;     /* [B,K,R], [B,K,A], [B,K] or NULL */
    const float *drop_xt, *drop_h, *drop_fake, *drop_fr, *drop_ho, *drop_out;   /* [T,N,E|R|R|E|E|R] keep masks or NULL */
    const float *drop_tile;                  /* [T,N,K+1,A] injected keep mask of the tanh tile, or NULL */
    float tile_p; uint64_t tile_seed;        /* drop_tile NULL and tile_p > 0: the tile mask is drawn inside the kernels */
    int mode; float temperature; const float *gumbel; uint64_t seed;
    const int64_t *forced; int forced_ld; int teacher;
    const uint8_t *ss_mode;                  /* as capmi_att2in2_rollout */
    float *h, *c;                            /* [T+1,N,R]  slot 0 = zero state, slot t+1 after step t */
    float *x;                                /* [T,N,E] */
    int64_t *it_all;                         /* [T,N] */
    float *xin;                              /* [T,N,G+R] teacher forcing: the xw product of all steps (one GEMM), or NULL */
    float *saved;                            /* [T,N,G+R] */
    float *h_drop, *fake_drop;               /* [T,N,R] */
    float *fr, *ho_t, *ho;                   /* [T,N,E]: fr after ReLU and mask, ho before / after its mask */
    float *fr_e, *ho_e;                      /* [T,N,A] */
    float *pi, *ctx;                         /* [T,N,K+1], [T,N,R] (context + ho) */
    float *out_t, *out_drop;                 /* [T,N,R] core output before / after its mask */
    int64_t *seq; float *seq_logp; float *sel_logp; uint8_t *live;   /* [N,L], [N,L,V1], [N,L], [N,L] */
    int64_t *it; uint8_t *unfinished;
    float *partial; int64_t partial_capacity;
} capmi_adaatt_rollout;

typedef struct capmi_adaatt_grads {
    float *embed, *w2h_w, *r_w2h_w, *h2h_w, *r_h2h_w;
    float *gate_b;                           /* [G+R]: the gradient of each of the three biases behind a gate column */
    float *d_fc_gates;                       /* [B,G+R]: for the v2h / r_v2h / fc_embed backward of the prefill */
    float *fr_w, *fr_b, *ho_w, *ho_b, *fre_w, *fre_b, *hoe_w, *hoe_b, *alpha_w, *alpha_b, *att2h_w, *att2h_b, *logit_w, *logit_b;
    float *d_att, *d_p_att;                  /* [B,K,R], [B,K,A] */
} capmi_adaatt_grads;

typedef struct capmi_adaatt_bwd_scratch {
    float *dlogits;                          /* [T,N,V1] */
    float *d_out, *d_ctx;                    /* [T,N,R] */
    float *d_e;                              /* [T,N,K+1] */
    float *d_hoe, *d_fre;                    /* [T,N,A] */
    float *d_fr, *d_ho;                      /* [T,N,E] */
    float *d_hdrop, *d_fakedrop;             /* [T,N,R] */
    float *d_sums;                           /* [T,N,G+R] */
    float *dc;                               /* [2][N,R] */
    float *d_x;                              /* [T,N,E] */
    float *partial; int64_t partial_capacity;
    const capmi_sparse_logp_grad *sparse;    /* as in capmi_updown_bwd_scratch */
} capmi_adaatt_bwd_scratch;

/* AttModel._forward / _sample over AdaAttCore: one host call per rollout, no host sync (select modes, CAPMI_SELECT_RAW, injected
 * Gumbel noise and ss_mode as capmi_att2in2_rollout_fwd), and the BPTT autograd would have recorded for it. */
int capmi_adaatt_rollout_fwd(const capmi_adaatt_weights *w, capmi_adaatt_rollout *r, void *stream);
int capmi_adaatt_rollout_bwd(const capmi_adaatt_weights *w, const capmi_adaatt_rollout *r, const float *g_seq_logp,
                             capmi_adaatt_bwd_scratch *s, capmi_adaatt_grads *g, void *stream);

/* one decode step in eval numerics (AttModel.get_logprobs_state up to the logits), as capmi_att2in2_decode_step */
typedef struct capmi_adaatt_step {
    int B, K, A, R, E, V1, maxout;
    const float *fc_gates, *att, *p_att, *att_mask;   /* [B,G+R], [B,K,R], [B,K,A], [B,K] or NULL */
    const int64_t *it;                       /* [rows] input tokens */
    float *xt, *saved, *h_drop, *fake_drop, *fr, *ho_t, *ho, *fr_e, *ho_e, *pi, *ctx, *out_t, *out_drop, *logits;
    float *partial; int64_t partial_capacity;
} capmi_adaatt_step;
int capmi_adaatt_decode_step(const capmi_adaatt_weights *w, capmi_adaatt_step *s, int rows, int rows_per_image,
                             const float *h_src, const float *c_src, float *h_dst, float *c_dst, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Test-time ensemble: the mixture log-probability of M members (AttEnsemble.get_logprobs_state, AttEnsemble.py:45-53,
 *   logprobs = log( sum_i w_i * softmax(logit_i) / sum_i w_i ) ).  For every row r:
 *   lse_i     = logsumexp_v in_i[r, v]            (each member is normalised here: logits and log-probs give the same result)
 *   out[r, v] = log sum_{i: w_i > 0} w_i * exp(in_i[r, v] - lse_i)
 * computed in log space, as m + log sum_i exp(a_i - m) with a_i = (in_i - max_i) - log(sum_i) + log w_i.  Difference from the
 * reference: its fp32 softmax -> weighted sum -> log underflows to -inf where every member's probability is below ~1e-38; here
 * the output stays finite.  A column is -inf only where it is -inf in every member with weight; NaN propagates (a member row
 * that is -inf everywhere gives NaN, as the reference's softmax does).  Members with weight 0 are not read.
 * rows == 0: success, nothing launched.  CAPMI_EINVAL: M outside 1..CAPMI_ENSEMBLE_MAX, V1 <= 0, ld_in or ld_out below V1,
 * a NULL pointer, a negative or non-finite weight, no positive weight, out overlapping an input.
 * One workgroup per row, two sweeps over the member rows (float4 loads); the weights are used as given (the caller
 * normalises them; log w_i is only an offset, so unnormalised weights shift the output by log sum_i w_i).
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_ENSEMBLE_MAX 8
typedef struct capmi_ensemble {
    int M, rows, V1, ld_in, ld_out;
    const float *in[CAPMI_ENSEMBLE_MAX];   /* member i: rows x V1 logits OR log-probs, row stride ld_in */
    float w[CAPMI_ENSEMBLE_MAX];           /* >= 0, normalised by the caller (sum 1) */
    float *out;                            /* rows x V1, row stride ld_out; may not alias an input */
} capmi_ensemble;
int capmi_ensemble_logprobs(const capmi_ensemble *e, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Discriminative decoding (disc.py): the row a search sees for a hypothesis whose token history was stepped under the target image
 * (slot 0) and under up to CAPMI_DISC_MAX - 1 distractor images (slots 1 .. D1 - 1).  For hypothesis (b, j), j < cur, with
 *   l_i[v] = in[(b * D1 + i) * cur + j, v] - logsumexp_v in[(b * D1 + i) * cur + j, v]     (every slot is normalised here)
 *   lt = l_0, P = {i >= 1 : present[b, i]}, D' = |P|, w = 1 - lambda:
 *   mode 0 (suppress): out[b * cur + j, v] = lt[v] - w * (logsumexp_{i in P} l_i[v] - log D')
 *   mode 1 (listener): out[b * cur + j, v] = lt[v] + w * (lt[v] - logsumexp_{i in P or i = 0} l_i[v])
 *   D' = 0 or lambda = 1: out = lt (the slots behind the target are not read).
 * The sum over the slots runs in log space, m + log sum_i exp(l_i - m): a column that is tiny under every distractor stays finite,
 * and for finite inputs the output is finite.  lt[v] = -inf gives -inf.  A column that is -inf under every distractor of P (and
 * finite under the target) gives +inf in mode 0 -- no distractor can say the word -- and lt[v] in mode 1.  NaN propagates.
 * Absent slots (present == 0) are not read; present[b, 0] is taken as 1.
 * rows == 0 (B or cur 0): success, nothing launched.  CAPMI_EINVAL: D1 outside 1..CAPMI_DISC_MAX, a negative B or cur, V1 <= 0,
 * ld_in or ld_out below V1, a mode other than 0 / 1, a NULL pointer, lambda outside [0, 1] or not finite, out overlapping in.
 * One workgroup per hypothesis, two sweeps over its present slot rows (float4 loads when the slot rows share their alignment mod
 * 16 bytes, i.e. cur * ld_in is a multiple of 4 or D1 = 1); no atomics, the result does not depend on arrival order.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_DISC_MAX 8
typedef struct capmi_disc {
    int B, D1, cur, V1, ld_in, ld_out, mode;   /* D1 = 1 + D slots per image; mode 0 suppress, 1 listener */
    float lambda;
    const float *in;          /* [B * D1 * cur, V1] logits, slot-major as above, row stride ld_in */
    const uint8_t *present;   /* [B, D1]; column 0 is the target and must be 1 */
    float *out;               /* [B * cur, V1], row stride ld_out; may not overlap in */
} capmi_disc;
int capmi_disc_combine(const capmi_disc *d, void *stream);

/* ---------------------------------------------------------------------------------------------
 * PPO structure loss (PPOLoss.forward, captioning/modules/losses.py:267-357): a clipped policy ratio plus a KL penalty against a
 * frozen old policy, over the N = B * n sampled rows of one rollout (n samples per image, image-major).  Row (i, t), t < L:
 *   m[i,t]  = 1 for t == 0, else (seq[i, t-1] > 0)                           (the end step still counts)
 *   A[i]    = scores[i] - (sum_k scores[img(i), k] - scores[i]) / (n - 1)     (leave-one-out baseline, new_self_critical's)
 *   r       = exp(ln[s] - lo[s]),  s = seq[i, t]                              (ln: lp_new row, lo: lp_old row)
 *   pg      = max(-A r, -A clamp(r, 1 - eps, 1 + eps))                       (NaN if either side is NaN, as torch.maximum)
 *   kl      = sum_v exp(lo[v]) (lo[v] - ln[v])                                 (F.kl_div(ln, lo, log_target=True).sum(-1))
 * masked means (M = sum m): out = {pg_loss, kl_loss, clipfrac = mean(|r - 1| > eps), loss = pg_loss + kl_coef kl_loss}; with
 * per_row ('none'): loss_rows[i] = sum_t (pg + kl_coef kl) m / sum_t m as well.
 *
 * capmi_ppo_loss_fwd: two launches (one workgroup per row reading the new and the old row once, float4 body; one workgroup for
 *   the means in double).  Writes row_stats [4][N*L] = {kl, r, pg, g_pg} with g_pg = d pg / d ln[s]:
 *     -A r where the unclipped side is the larger, -A r [1-eps <= r <= 1+eps] where the clamped side is, the mean of the two on a
 *     tie (torch.maximum's backward; while the clamp is inactive the two sides tie).  The side that gets no gradient adds nothing:
 *     r = inf with A > 0 gives pg = -A (1 + eps), finite, and g_pg = 0.  (The reference's fp32 autograd forms 0 * inf = NaN in
 *     exp's backward there; 0 is the limit of the finite case.)
 *   and msum: M ([1], 'mean') or sum_t m per sample ([N], per_row).
 *   Masked rows (m = 0) are not read; their row_stats are 0.  The reference multiplies them by 0, so the two differ only where a
 *   masked row holds an infinity or a NaN (the reference then gives NaN).  Everything else follows IEEE as the reference's fp32
 *   ops do: a -inf in an old row gives a NaN kl (0 * -inf), a -inf new entry under a positive old probability an infinite kl.
 *   A token outside [0, V1) gives r = NaN and is not read.
 * capmi_ppo_loss_bwd: one launch, one workgroup per row; reads the old row, g_pg, msum and the upstream gradient g_out ([1] for
 *   'mean': a device scalar, no host sync; [N] for per_row) and writes the dense gradient once:
 *     grad[i,t,v] = c (-kl_coef exp(lo[v]) + [v == s] g_pg),  c = g_out m / M;  masked rows are written as zeros.
 * Both: lp_new / lp_old / grad are [N*L, V1] row views with strides ld_new / ld_old / ld_grad (>= V1, 4-byte aligned), seq [N, L]
 * int64 contiguous, scores [N] float.  N == 0: success, nothing launched.  CAPMI_EINVAL: n < 2, N not a multiple of n, L or V1
 * below 1, a stride below V1, a NULL pointer that the call reads or writes, eps or kl_coef negative / not finite, row_stats
 * overlapping an input row span, grad overlapping the old rows.
 * ------------------------------------------------------------------------------------------- */
typedef struct capmi_ppo {
    int N, L, V1, n;                 /* rows N*L; n samples per image */
    int ld_new, ld_old, ld_grad;     /* row strides, floats */
    int per_row;                     /* 0: reduction 'mean', 1: 'none' */
    float eps, kl_coef;              /* ppo_cliprange, ppo_kl_coef */
    const float *lp_new;             /* [N*L, V1] the rollout's output (fwd) */
    const float *lp_old;             /* [N*L, V1] the old policy's log-probs */
    const int64_t *seq;              /* [N, L] sampled tokens */
    const float *scores;             /* [N] rewards (fwd) */
    float *row_stats;                /* [4][N*L] kl, r, pg, g_pg (written by fwd, read by bwd) */
    float *msum;                     /* [1] or [N] mask sums (written by fwd, read by bwd) */
    float *out;                      /* [4] pg_loss, kl_loss, clipfrac, loss (fwd) */
    float *loss_rows;                /* [N] per_row losses (fwd, per_row only) */
    const float *g_out;              /* [1] or [N] upstream gradient (bwd) */
    float *grad;                     /* [N*L, V1] d loss / d lp_new (bwd) */
} capmi_ppo;
int capmi_ppo_loss_fwd(const capmi_ppo *p, void *stream);
int capmi_ppo_loss_bwd(const capmi_ppo *p, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-entropy criteria of the teacher-forced pass (captioning/modules/losses.py:204-265): LanguageModelCriterion
 * (smoothing == 0) and LabelSmoothing (0 < smoothing < 1) over the log-probs logp [N, T, V1] (float, contiguous), the targets
 * tok [N, tok_ld] int64 and the mask [N, mask_ld] float, tok_ld, mask_ld >= T: both criteria cut labels and masks to the T
 * columns of the input (target[:, :T]); the uncut buffers are read through their row pitch, nothing is copied.
 * Position (n, t), with s = tok[n, t] and m = mask[n, t]:
 *   smoothing == 0:  c = -logp[n,t,s] m                                   (one entry gathered; the dense row is not read)
 *   smoothing  > 0:  c = (ent - off sum_v logp[n,t,v] - (conf - off) logp[n,t,s]) m
 *                    off = smoothing / (V1 - 1), conf = 1 - smoothing, ent = (V1-1) off ln off + conf ln conf = sum_v q ln q of the
 *                    smoothed target distribution q (the three are formed in double on the host and passed by value)
 *   loss = sum c / sum m ([1], 'mean');  per_row ('none', the drop_worst route): loss[n] = sum_t c / sum_t m ([N]).
 * A position with m == 0 is not read and contributes an exact 0; a mask sum of 0 gives 0 / 0 = NaN as the reference does.  A token
 * outside [0, V1) is not read and gives NaN.
 *
 * capmi_xe_loss_fwd: two launches, no float atomics.  Stage 1 writes c to pos [N*T]: one thread per position without smoothing;
 *   with it one workgroup per (n, t) row, the row read once (scalar head up to the 16-byte boundary, float4 body, scalar tail:
 *   V1 is odd in general, so row bases fall off the boundary).  Stage 2, one workgroup, folds pos and the mask in double in a
 *   fixed order and writes loss and msum (the mask sums the backward needs: [1], or [N] with per_row).  Two runs on the same
 *   inputs are bit-equal.
 * capmi_xe_loss_bwd: one launch over [N, T]; writes the gradient in the sparse form of capmi_sparse_logp_grad:
 *     g_sel[n,t] = -(conf - off) m / msum u      (d loss / d logp[n,t,s])
 *     g_sum[n,t] = -off m / msum u               (d loss / d sum_v logp[n,t,v]; smoothing > 0 only, else g_sum is not written)
 *   msum = msum[0] ('mean') or msum[n] (per_row); u = g_out[0] / g_out[n], the upstream gradient on the device, or 1 when g_out
 *   is NULL (a scalar loss hands its upstream gradient on as capmi_sparse_logp_grad.scale, no host read).  No dense [N, T, V1]
 *   gradient is produced.
 * CAPMI_EINVAL: a NULL pointer that the call reads or writes, N, T or V1 <= 0, a pitch below T, smoothing outside [0, 1),
 * smoothing > 0 with V1 < 2.
 * ------------------------------------------------------------------------------------------- */
typedef struct capmi_xe_loss {
    int N, T, V1;
    int tok_ld, mask_ld;             /* row pitches of tok / mask, elements, >= T */
    int per_row;                     /* 0: reduction 'mean', 1: 'none' */
    double smoothing;                /* 0: LanguageModelCriterion; (0, 1): LabelSmoothing */
    const float *logp;               /* [N, T, V1] (fwd) */
    const int64_t *tok;              /* [N, tok_ld] targets (fwd) */
    const float *mask;               /* [N, mask_ld] */
    float *pos;                      /* [N*T] scratch: the per-position values (fwd) */
    float *msum;                     /* [1] or [N] mask sums (written by fwd, read by bwd) */
    float *loss;                     /* [1] or [N] (fwd) */
    const float *g_out;              /* NULL, or [1] / [N] upstream gradient (bwd) */
    float *g_sel;                    /* [N*T] (bwd) */
    float *g_sum;                    /* [N*T] (bwd, smoothing > 0) */
} capmi_xe_loss;
int capmi_xe_loss_fwd(const capmi_xe_loss *p, void *stream);
int capmi_xe_loss_bwd(const capmi_xe_loss *p, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Knowledge distillation (distill.hip; losses.DistillCriterion): the hard-label NLL of the teacher-forced pass mixed with the
 * temperature-softened KL(teacher || student) over the whole vocabulary.  There is no reference counterpart: the formula below is
 * normative (tests/distill_ref64.py restates it in float64).  Position (i, t), t < T, with the student row ls = lp_s[i, t, :],
 * the teacher row lt = lp_t[i, t, :], s = tok[i, t], m = mask[i, t], lambda in [0, 1], tau > 0:
 *   a = ls / tau, b = lt / tau, pS = softmax(a), pT = softmax(b)
 *   kl   = sum_v pT_v (log pT_v - log pS_v)                       (a term with pT_v == 0 is exactly 0)
 *   c    = m ((1 - lambda) (-ls_s) + lambda tau^2 kl)
 *   loss = sum c / sum m ('mean');  per_row ('none', the drop_worst route): loss_rows[i] = sum_t c / sum_t m
 *   d loss / d ls_v = g m / M (-(1 - lambda) [v == s] + lambda tau (pS_v - pT_v))
 * A position with m == 0 is not read, contributes an exact 0 and gets a gradient row of zeros; a mask sum of 0 gives 0 / 0 = NaN as
 * the other criteria do; a token outside [0, V1) gives NaN and is not read (its gradient row has no hard-label term).
 * Rows are addressed through strides: student row (i, t) at lp_s + (i T + t) ld_s, teacher row at lp_t + (i t_rows + t) ld_t (the
 * teacher may be the [:, :T] cut of a longer [N, t_rows, .] tensor), gradient row at grad + (i T + t) ld_grad.
 *
 * capmi_distill_loss_fwd: two launches, no float atomics; two runs on the same inputs are bit-equal.  (1) one workgroup per (i, t)
 *   row reads the student and the teacher row once, in one sweep (scalar head up to the 16-byte boundary, float4 body, scalar
 *   tail where both rows share their alignment mod 16 bytes, else scalar): an online-rescaled running max and sum for both rows
 *   and the running sum_v e^(b_v - max) (b_v - a_v), so that kl = that / zT - lseT + lseS takes no second pass.  Writes
 *   row_stats [4][N*T] = {lseS, lseT, kl, -ls_s} (lse of the tempered rows; masked positions: zeros).  (2) one workgroup folds them
 *   in double in a fixed order: out [3] = {lm_loss = masked mean of -ls_s, kd_loss = masked mean of kl (before lambda and tau^2),
 *   loss}, msum ([1], or [N] with per_row) and, with per_row, loss_rows [N].
 * capmi_distill_loss_bwd: one launch, one workgroup per row; reads both rows, row_stats, msum and the upstream gradient g_out ([1]
 *   for 'mean': a device scalar, no host sync; [N] for per_row) and writes the dense gradient once, with plain stores: the
 *   teacher-forced backward reads it next.  lambda == 0 reads neither row.
 * CAPMI_EINVAL: tau <= 0 or not finite, lambda outside [0, 1], a stride below V1, t_rows, tok_ld or mask_ld below T, N < 0, T or
 * V1 below 1, a NULL pointer that the call reads or writes, a pointer off 4 bytes.  N == 0: success, nothing launched.
 * ------------------------------------------------------------------------------------------- */
typedef struct capmi_distill {
    int N, T, V1;
    int ld_s, ld_t, ld_grad;         /* row strides, floats, >= V1 */
    int t_rows;                      /* rows per sample of the teacher tensor, >= T */
    int tok_ld, mask_ld;             /* row pitches of tok / mask, elements, >= T */
    int per_row;                     /* 0: reduction 'mean', 1: 'none' */
    float lambda, tau;               /* distill_weight, distill_temperature */
    const float *lp_s;               /* [N*T, V1] the student's teacher-forced log-probs */
    const float *lp_t;               /* [N, t_rows, V1] the teacher's log-probs */
    const int64_t *tok;              /* [N, tok_ld] targets */
    const float *mask;               /* [N, mask_ld] */
    float *row_stats;                /* [4][N*T] lseS, lseT, kl, -ls_s (written by fwd, read by bwd) */
    float *msum;                     /* [1] or [N] mask sums (written by fwd, read by bwd) */
    float *out;                      /* [3] lm_loss, kd_loss, loss (fwd) */
    float *loss_rows;                /* [N] per_row losses (fwd, per_row only) */
    const float *g_out;              /* [1] or [N] upstream gradient (bwd) */
    float *grad;                     /* [N*T, V1] d loss / d lp_s (bwd) */
} capmi_distill;
int capmi_distill_loss_fwd(const capmi_distill *p, void *stream);
int capmi_distill_loss_bwd(const capmi_distill *p, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Corpus language evaluation without Java: coco-caption's Cider, Bleu (option 'closest') and Rouge over token ids, for the
 * validation pass (eval_utils.language_eval -> lang_stats['CIDEr'], 'Bleu_1'..'Bleu_4', 'ROUGE_L').  A caption is the tokens of
 * its int64 row before the first 0 (the whole row when it holds none); ids are below 65535.  Restated from the published
 * formulas (coco-caption is not part of the reference checkout: PARITY UNPINNED, see tests/langeval_ref64.py).
 *
 * The references of a split are ragged: refs [total_refs, ref_w], image i owns rows ref_off[i] .. ref_off[i+1].
 *   CIDEr    df(g) = number of images with n-gram g in any reference (counted once per image); idf(g) = log(n_img) - log(max(1, df));
 *            vec = tf * idf per n-gram, per order n = 1..4 the cosine of hypothesis and reference (raw dot product where a norm is
 *            0); image score = 10 * mean_n mean_ref cosine.  No clipping, no length penalty.  Corpus: mean over the added images.
 *   BLEU     per image and n: guess = max(0, len - n + 1), correct = sum_g min(tf_hyp(g), max_ref tf_ref(g)); testlen = len, reflen =
 *            the reference length closest to len (ties: the shorter).  Corpus: integer sums over the added images, then
 *            p_n = (correct_n + 1e-15) / (guess_n + 1e-9), Bleu_n = (p_1 .. p_n)^(1/n), times exp(1 - 1/ratio) when
 *            ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1.
 *   ROUGE_L  lcs against every reference; P = max lcs / len_hyp, R = max lcs / len_ref, F = (1 + b^2) P R / (R + b^2 P), b = 1.2
 *            (0 when P or R is 0 -- an empty hypothesis scores 0).  Corpus: mean over the added images.
 * Float arithmetic is double.
 *
 * capmi_langeval_build: two launches.  (1) one workgroup per image inserts its DISTINCT reference n-grams (first occurrence in
 *   (reference, position) order: the same n-grams on every run) into table_keys / table_counts with atomicCAS / atomicAdd --
 *   open addressing, linear probing, keys and hash of capmi_ciderd_score; both arrays zeroed by the caller, table_cap a power of
 *   two.  (2) one workgroup per reference writes ref_norm [total_refs, 4].
 * capmi_langeval_add: one launch, one workgroup per hypothesis row: hyp [H, L] int64, img_idx [H] int64 (which image each row
 *   describes, any order).  Writes cider / rouge / bleu_stats / lens / lcs of those images and seen = 1; a later row for an image
 *   replaces an earlier one (within one call too).  No host sync.
 * capmi_langeval_reduce: one launch, one workgroup: out [8] = Bleu_1..4, ROUGE_L, CIDEr, number of images added, error bits;
 *   totals [10] = guess_1..4, correct_1..4, testlen, reflen (int64 sums, the same bits whatever the order of the adds).
 * err [1] (zeroed by the caller) collects CAPMI_LANGEVAL_E_*; the results are meaningless when it is not 0.
 * CAPMI_EINVAL: a NULL pointer, n_img < 1, ref_w or L outside 1..CAPMI_LANGEVAL_LMAX (rows are never truncated), table_cap not a
 * power of two.  H == 0: success, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_LANGEVAL_LMAX 64
#define CAPMI_LANGEVAL_E_TABLE_FULL 1   /* more distinct n-grams than table_cap */
#define CAPMI_LANGEVAL_E_TOKEN 2        /* a token id outside [0, 65535) */
#define CAPMI_LANGEVAL_E_IMAGE 4        /* an image index outside [0, n_img) */
typedef struct capmi_langeval {
    int n_img, total_refs, ref_w;
    const int64_t *refs;                     /* [total_refs, ref_w] */
    const int32_t *ref_off;                  /* [n_img + 1] */
    uint64_t *table_keys;                    /* [table_cap], empty slot = 0 */
    int32_t *table_counts;                   /* [table_cap] document frequencies */
    uint32_t table_cap;
    double *ref_norm;                        /* [total_refs, 4] */
    double *cider, *rouge;                   /* [n_img] */
    int32_t *bleu_stats;                     /* [n_img, 4, 2] guess, correct */
    int32_t *lens;                           /* [n_img, 2] testlen, reflen */
    int32_t *lcs;                            /* [total_refs] lcs of the image's hypothesis and each reference */
    int32_t *seen;                           /* [n_img] 1 once the image has a hypothesis */
    int32_t *err;                            /* [1] */
} capmi_langeval;
int capmi_langeval_build(const capmi_langeval *e, void *stream);
int capmi_langeval_add(const capmi_langeval *e, const int64_t *hyp, int H, int L, const int64_t *img_idx, void *stream);
int capmi_langeval_reduce(const capmi_langeval *e, double *out, int64_t *totals, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Diversity evaluation of n sampled captions per image (eval_multi.eval_div_stats / eval_self_cider / eval_oracle), on the
 * tables of a capmi_langeval.  Captions are token-id rows as above; 2 <= n <= CAPMI_DIVEVAL_NMAX.  div_utils.py is pinned by
 * tests/golden/diveval_ref.npz; mBLEU and self-CIDEr are restated (PARITY UNPINNED, tests/diveval_ref64.py).  Double throughout.
 *   Div1, Div2  per image: distinct k-grams over the n captions / (1e-6 + tokens of the n captions), k = 1, 2 (the denominator is
 *               the token count for k = 2 too).  Corpus: mean over the added images.
 *   gDiv1       distinct unigrams over every caption added since the bitmap was zeroed (replaced groups included).
 *   mBLeu_1..4  per slot i the corpus Bleu ('closest') of caption i against the image's other n-1 captions; the mean over i.
 *               sent_bleu2 [img, i]: bleu_scorer's per-instance Bleu_2 of the same counts.
 *   self_cider  K[i][j] = 10 * (1/4) sum_k cos_k(c_i, c_j) on the tf-idf vectors of the langeval table (an order with a zero norm
 *               contributes 0); i <= j computed, mirrored.  lambda = eigenvalues of K/10 clipped at 0:
 *               -log(sqrt(lambda_max) / sum sqrt(lambda)) / log(n); 0.0 when the sum is 0 (every caption empty; numpy gives NaN).
 *   oracle      (oracle != 0) every slot scored against the image's references exactly as capmi_langeval_add scores a hypothesis:
 *               oracle_scores [img, i, 6] = CIDEr, sentence Bleu_1..4, ROUGE_L.
 *
 * capmi_diveval_add: hyp [B * n, L] int64, rows k*n .. k*n+n-1 describe image img_idx[k].  Launches: (1) a workgroup per row: the
 *   four tf-idf norms; (2) a workgroup per row walks the image's n rows once: its row of K (upper triangle, mirrored), the clip
 *   counts and closest length of mBLEU, the n-grams no earlier position and no earlier slot holds (slot_distinct), atomicOr into
 *   vocab_bits; (3) with oracle, a workgroup per row against the references; (4) a wave per image: cyclic Jacobi on K/10 (row-cyclic
 *   sweeps until the off-diagonal square sum is <= (2^-52 trace)^2, at most CAPMI_DIVEVAL_SWEEPS), eig ascending, self_cider, the
 *   per-image sums.  A later group for an image replaces an earlier one (within one call too).  No host sync, no allocation.
 * capmi_diveval_reduce: one workgroup.  out [CAPMI_DIVEVAL_NOUT] = Div1, Div2, gDiv1, mBLeu_1..4, self_cider, images added, error
 *   bits, oracle_{CIDEr, Bleu_1..4, ROUGE_L}, avg_{the same}; totals [n, 10] = per slot guess_1..4, correct_1..4, testlen, reflen.
 *   Integers are summed as integers, floats in index order: the same bits whatever the order of the adds.
 * err collects CAPMI_LANGEVAL_E_*.  CAPMI_EINVAL: a NULL pointer, n outside 2..CAPMI_DIVEVAL_NMAX, L outside 1..CAPMI_LANGEVAL_LMAX,
 * an invalid table.  B == 0: success, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_DIVEVAL_NMAX 32
#define CAPMI_DIVEVAL_SWEEPS 30
#define CAPMI_DIVEVAL_NOUT 22
#define CAPMI_DIVEVAL_VOCAB_WORDS 2048   /* 65 536 bits */
typedef struct capmi_diveval {
    capmi_langeval lang;                     /* tables and references; with oracle its output pointers are the scratch
                                                [n_img * n] rows of cider / rouge / bleu_stats / lens, lcs and seen unused;
                                                lang.err must be err below */
    int n, oracle;
    double *norm;                            /* [n_img, n, 4] tf-idf norms of the captions */
    int32_t *slot_distinct;                  /* [n_img, n, 2] n-grams first seen in this slot, orders 1 and 2 */
    int32_t *distinct;                       /* [n_img, 2] */
    int32_t *tokens;                         /* [n_img] */
    int32_t *mbleu_stats;                    /* [n_img, n, 10] guess 1..4, correct 1..4, testlen, reflen */
    double *sent_bleu2;                      /* [n_img, n] */
    double *K;                               /* [n_img, n, n] */
    double *eig;                             /* [n_img, n] ascending */
    double *self_cider;                      /* [n_img] */
    double *oracle_scores;                   /* [n_img, n, 6] (oracle only) */
    int32_t *seen;                           /* [n_img] */
    int32_t *err;                            /* [1] */
    uint32_t *vocab_bits;                    /* [CAPMI_DIVEVAL_VOCAB_WORDS] */
} capmi_diveval;
int capmi_diveval_add(const capmi_diveval *d, const int64_t *hyp, int B, int L, const int64_t *img_idx, void *stream);
int capmi_diveval_reduce(const capmi_diveval *d, double *out, int64_t *totals, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sentence statistics of eval_utils.language_eval (eval_utils.py:27-36, 55-68, 79-80, 121): novel_sentences, vocab_size,
 * bad_count_rate and the mean perplexity / entropy, counted over token-id rows.  A SENTENCE is the tokens of a row before its
 * first 0 (all of them when it holds none); what follows the first 0 is ignored.  Rows are at most CAPMI_LANGEVAL_LMAX wide, ids
 * below 65535 (and, for generated rows, below V1).
 *
 * Two sets of sentences live in HBM as open-addressing tables of 64-bit words: the low 32 bits name a row (index + 1; 0 = empty
 * slot), the high 32 bits are the high half of the sentence's hash.  Membership is exact: a probe that meets an equal hash half
 * compares the tokens of the named row and goes on probing when they differ.  One wave per row, lane i holds token i.
 * hash = mix64(sum_i mix64((i + 1) << 16 | (token_i + 1)) + length) & hash_mask; hash_mask is ~0 in production (a test narrows
 * it to make unequal sentences collide).
 *
 * capmi_sentset_build: one launch, once per run.  train_rows [n_train, train_w] (int64 when train_elem == 8, uint32 when 4,
 *   zero-padded); every sentence that does not contain unk_id (unk_id <= 0: none is skipped) is inserted into train_table
 *   [train_cap] (zeroed by the caller, a power of two).  A duplicate finds its twin and takes no slot.
 * capmi_sentset_add: two launches.  seqs [rows, L] int64 on the device, the captions of one decoded batch; base_row: where the
 *   batch goes in gen_rows [gen_capacity, CAPMI_LANGEVAL_LMAX] (uint16, canonical: zero from the end of the sentence on).
 *   (1) stores the canonical rows and sets the bits of their tokens in vocab_bits [(V1 + 31) / 32] (token 0 excluded).
 *   (2) inserts every row into gen_table [gen_cap] with atomicCAS on the slot word: of equal sentences in flight exactly one
 *   wave sees the empty slot (the CAS returns 0) and counts; the others read the winner's word, find the winner's tokens in
 *   gen_rows -- stored by launch (1), hence in memory -- and leave.  The winner looks the sentence up in train_table; it is novel
 *   when it is missing there or contains unk_id.  counts [CAPMI_SENTSET_NCOUNT] (uint64): rows seen, distinct generated
 *   sentences, distinct generated sentences that are novel, rows of the single-caption pass, those that end in a bad ending.
 *   None depends on the order of arrival.
 * capmi_sentset_add_first: one launch, one workgroup, the single-caption pass: seq [rows, L] int64; counts the rows and the
 *   rows whose last token is in bad [n_bad] (an empty row counts 0); adds perplexity [rows] / entropy [rows] (float32, device) to
 *   sums [2] in double: thread t sums rows t, t + 256, ..., then the 256 partial sums in index order.
 * capmi_sentset_reduce: one launch: out [CAPMI_SENTSET_NOUT] = the five counts, popcount of vocab_bits, sum of perplexity, sum
 *   of entropy, error bits.
 * err [1] collects CAPMI_LANGEVAL_E_TABLE_FULL (either table) and CAPMI_LANGEVAL_E_TOKEN.  Calls only enqueue.  CAPMI_EINVAL: a
 * NULL pointer, a width outside 1..CAPMI_LANGEVAL_LMAX, a table size that is no power of two, train_elem not 4 or 8, V1 outside
 * 1..65536, rows beyond gen_capacity.  rows == 0: success, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_SENTSET_NCOUNT 5
#define CAPMI_SENTSET_NOUT 9
typedef struct capmi_sentset {
    int n_train, train_w, train_elem, unk_id;
    const void *train_rows;                  /* [n_train, train_w]; may be NULL when n_train == 0 */
    uint64_t *train_table;                   /* [train_cap] */
    uint32_t train_cap;
    int gen_capacity;
    uint16_t *gen_rows;                      /* [gen_capacity, CAPMI_LANGEVAL_LMAX]; may be NULL when gen_capacity == 0 */
    uint64_t *gen_table;                     /* [gen_cap] */
    uint32_t gen_cap;
    int V1;
    uint32_t *vocab_bits;                    /* [(V1 + 31) / 32] */
    const int64_t *bad;                      /* [n_bad]; may be NULL when n_bad == 0 */
    int n_bad;
    uint64_t *counts;                        /* [CAPMI_SENTSET_NCOUNT] */
    double *sums;                            /* [2] perplexity, entropy */
    int32_t *err;                            /* [1] */
    uint64_t hash_mask;
} capmi_sentset;
int capmi_sentset_build(const capmi_sentset *s, void *stream);
int capmi_sentset_add(const capmi_sentset *s, const int64_t *seqs, int rows, int L, int base_row, void *stream);
int capmi_sentset_add_first(const capmi_sentset *s, const int64_t *seq, int rows, int L, const float *perplexity,
                            const float *entropy, void *stream);
int capmi_sentset_reduce(const capmi_sentset *s, double *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The CIDEr-D document-frequency table of a caption corpus, built on the device (df_build.hip): what scripts/prepro_ngrams.py
 * computes with CiderScorer.compute_doc_freq and tools/convert_df.py turns into the image capmi_ciderd_score probes.
 *
 * The corpus is ragged: tok [total_tokens] (int32 when tok_elem == 4, int64 when 8), cap_off [n_caps + 1] (caption c is
 * tok[cap_off[c] .. cap_off[c + 1])), img_off [n_img + 1] (image i owns captions img_off[i] .. img_off[i + 1] - 1; it may own
 * none).  A caption is exactly its tokens, a 0 included: the caller appends the <eos>, nothing here stops at a 0 or adds one,
 * and no caption is cut at any width.
 *
 * capmi_df_count: one launch, one workgroup per image.  For n = 1..4, every n-gram that occurs in any caption of an image adds 1
 *   to its slot of the counting table (table_keys uint64 / table_counts int32 [table_cap], zeroed by the caller, a power of two),
 *   once per image however often it occurs there.  Keys and hash are the scorer's (16-bit fields of id + 1, splitmix64); a slot
 *   is claimed with atomicCAS on its key and linear probing, the count is an integer atomicAdd: the key -> count mapping is the
 *   same on every run, only the slots are not.  An occurrence counts when no EARLIER token position of the image starts the
 *   same n-gram; the earlier positions are walked in tiles through LDS, so an image may be of any size (the walk is quadratic
 *   in the image's tokens).  n_distinct [1] (zeroed by the caller) receives the number of slots claimed.
 * capmi_df_finalize: one launch.  Every occupied slot of the counting table is inserted into keys uint64 / vals float64 [cap]
 *   (zeroed by the caller, a power of two), vals = the count converted exactly.
 * err [1] (zeroed by the caller) collects CAPMI_LANGEVAL_E_TABLE_FULL (either table), CAPMI_LANGEVAL_E_TOKEN (an id outside
 * [0, 65535); it counts as id 0) and CAPMI_DF_E_OFFSETS (an image whose offsets decrease or leave [0, n_caps] / [0, total_tokens],
 * or img_off that does not run from 0 to n_caps; the image is skipped).  Nothing is read or written out of range in any of these
 * cases; the tables are meaningless when err is not 0.
 * cap_off_host / img_off_host: the same offsets in host memory, or NULL.  Where given they are checked before anything is
 * launched (the kernel reads the device copies).  Calls only enqueue and never allocate.
 * CAPMI_EINVAL: a NULL pointer (tok may be NULL when total_tokens == 0), tok_elem not 4 or 8, a negative size, a table size that is
 * no power of two, host offsets that decrease or do not run from 0 to n_caps / total_tokens.  n_img == 0: success, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_DF_E_OFFSETS 8            /* malformed cap_off / img_off (joins CAPMI_LANGEVAL_E_*) */
int capmi_df_count(const void *tok, int tok_elem, int64_t total_tokens, const int64_t *cap_off, const int64_t *cap_off_host,
                   int64_t n_caps, const int64_t *img_off, const int64_t *img_off_host, int n_img, uint64_t *table_keys,
                   int32_t *table_counts, uint32_t table_cap, uint32_t *n_distinct, int32_t *err, void *stream);
int capmi_df_finalize(const uint64_t *count_keys, const int32_t *counts, uint32_t count_cap, uint64_t *keys, double *vals,
                      uint32_t cap, int32_t *err, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Store rows of a block of images, built on the device (region_rows.hip): norm_att_feat, the box-geometry columns of use_box,
 * norm_box_feat and the re-ordering of an image's rows by the last column (captioning/data/dataloader.py:266-282).  One launch,
 * one workgroup per image.
 *   src    [sum K, D] float32, the region rows as the feature files hold them; image i owns rows first_i .. first_i + K_i - 1
 *   boxes  [sum K, 4] float32 x1, y1, x2, y2 of the same rows (read with use_box only; may be NULL without it)
 *   table  [n_images, 4] int32 on the DEVICE: first row, K, height, width; table_host: the same words in host memory -- the
 *          arguments are checked there, the kernel reads the device copy
 *   dst    rows of D + 5 * use_box floats, leading dimension ldd (in floats): image i's rows go to dst rows first_i .. first_i + K_i - 1,
 *          nothing else is written (the ldd - row elements between two rows are left alone).  No alignment beyond 4 bytes is asked of
 *          src, boxes or dst.
 *   norm_att: every row of src is divided by its L2 norm over D.
 *   use_box:  the columns x1 / w, y1 / h, x2 / w, y2 / h, ((x2 - x1) * (y2 - y1)) / (w * h) are appended, in float32 with correctly
 *          rounded, non-contracted operations in that order (w, h and the integer w * h converted to float first): bit for bit
 *          what numpy computes in float32.  norm_box divides the five columns by their L2 norm.  The K rows are then written in the
 *          order of the last column, descending, equal keys in file order (Python's stable sorted(..., reverse=True)).  NaN keys go
 *          behind every other key, in file order; they are not refused (that would take a device-to-host wait).
 * CAPMI_EINVAL, before anything is launched: a NULL src / table_host / table / dst (boxes with use_box), n_images <= 0, D <= 0,
 * a first row < 0 or K <= 0, with use_box K > CAPMI_REGION_KMAX or height / width <= 0, ldd < D + 5 * use_box, a pointer off 4 bytes.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_REGION_KMAX 1024
int capmi_region_rows_build(const float *src, const float *boxes, const int32_t *table_host, const int32_t *table, int n_images,
                            int D, float *dst, int64_t ldd, int norm_att, int use_box, int norm_box, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The compact resident feature store (resident.hip; captioning/data/resident.py): region rows kept in HBM as float32, bfloat16 or
 * IEEE half, and the launch that turns the store into a batch.
 * capmi_rows_narrow: dst[i] = src[i] converted to CAPMI_ROWS_BF16 or CAPMI_ROWS_FP16, round to nearest even, i < count.  NaN stays NaN
 *          (quiet), +-inf stays +-inf; fp16 overflow goes to +-inf and fp16 subnormals are produced: the bits of
 *          torch.Tensor.to(dtype).  src: 4-byte aligned (the fp32 staging block of an insert), dst: 2-byte aligned -- any row of the
 *          store: a scalar head up to dst's first 16-byte boundary, 16-byte stores, a scalar tail.
 *          CAPMI_EINVAL: a NULL pointer, count <= 0, a dtype other than the two, src off 4 bytes, dst off 2.
 * capmi_resident_gather: one launch, one workgroup per output row.
 *   rows   the store, [n_rows, F] elements of `dtype` (CAPMI_ROWS_F32: a plain copy), rows packed (leading dimension F)
 *   table  [B, 2] int32 on the DEVICE: (first row, K) per batch image, K = 0: not resident (first is not read); table_host: the same
 *          words in host memory -- the arguments are checked there, the kernel reads the device copy (as capmi_region_rows_build)
 *   att    [B, kmax, F] float32: att[b, k, :] = row first_b + k widened (exact) for k < K_b, +0.0 for k >= K_b
 *   mask   [B, kmax] float32: 1 for k < K_b, else 0
 *   No alignment beyond the element size is asked of rows, beyond 4 bytes of att: the 16-byte stores follow each output row, the
 *   loads take the widest form the source row's address allows, down to single elements (F = 2053: 4106-byte rows at 16 bits).
 *   The caller guarantees first_b + K_b <= n_rows.
 *   CAPMI_EINVAL, before anything is launched: a NULL pointer, B / kmax / F <= 0, an unknown dtype, K < 0 or K > kmax, first < 0
 *   where K > 0, a pointer off its element size.
 * capmi_rows_l2norm: norm_att_feat for rows on their way into the store, in place: every row of rows [n_rows, D] (packed) over its L2
 *          norm, the squares summed in the order of numpy's float32 add.reduce (8 strided accumulators per run of up to 128, runs
 *          split at n / 2 rounded down to 8), every operation a correctly rounded float32 one: the bits of
 *          att / np.linalg.norm(att, 2, 1, keepdims=True), the loader's host path.  A zero row becomes NaN, as there.
 *          CAPMI_EINVAL: NULL, n_rows <= 0, D <= 0 or D > CAPMI_ROWS_L2NORM_DMAX, rows off 4 bytes.
 * ------------------------------------------------------------------------------------------- */
#define CAPMI_ROWS_F32 0
#define CAPMI_ROWS_BF16 1
#define CAPMI_ROWS_FP16 2
#define CAPMI_ROWS_L2NORM_DMAX 8192
int capmi_rows_l2norm(float *rows, int64_t n_rows, int D, void *stream);
int capmi_rows_narrow(const float *src, void *dst, int64_t count, int dtype, void *stream);
int capmi_resident_gather(const void *rows, int dtype, int F, const int32_t *table_host, const int32_t *table, int B, int kmax,
                          float *att, float *mask, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm1d over the valid region rows (region_norm.hip; use_bn, AttModel.py:80-85 under pack_wrapper :44-49).
 *   x / y / dy / dx  [rows, D] float32, rows = B * K; mask: one float per row, 0 = padded region (NULL: every row is valid)
 *   M, the number of valid rows, is counted on the device; nothing here waits for the device.
 * capmi_bn_row_blocks(rows): row blocks nrb of the statistics / backward partials.
 * capmi_bn_stats:    partial [nrb][2][D] (mean minus the pivot -- the column's value in the first valid row --, sum of squared deviations
 *                    of the block's valid rows), then nrb valid-row counts: nrb * (2 * D + 1) floats.  One read of x, no atomics.
 * capmi_bn_finalize: x / mask / rows: those of capmi_bn_stats (the pivot row is read again; x may be NULL with train == 0).
 *                    train != 0: merges the blocks in block order (Chan et al.) -> mean [D], rstd [D] = 1 / sqrt(biased var + eps),
 *                    count [1] = M; running_mean / running_var (unbiased variance, `momentum`) and num_batches_tracked (+1) are
 *                    updated in place (NULL: not kept).  M < 2: mean / rstd are those of the M rows (variance 0), the running buffers
 *                    and the counter are left alone.  train == 0: mean = running_mean, rstd = 1 / sqrt(running_var + eps), count = 0,
 *                    partial is not read, nothing is updated.
 *                    Either way shift [2][D] receives the mean as a pair: the pivot (0 in eval mode) and the mean minus the pivot.
 * capmi_bn_apply:    y = ((x - shift[0]) - shift[1]) * rstd * gamma + beta on valid rows, 0 on padded rows.  y may be x.
 * capmi_bn_bwd_partial: partial [nrb][2][D]: per row block sum dy and sum dy * xhat over the valid rows.
 * capmi_bn_colsum_parts: out0 / out1 [D] (either may be NULL) = the sums of partial[p][0] / partial[p][1] over p < nparts, in order.
 * capmi_bn_bwd_dx:   train: dx = gamma * rstd * (dy - (dbeta + xhat * dgamma) / count) on valid rows; eval: gamma * rstd * dy; 0 on
 *                    padded rows.  dx may be dy.
 * capmi_bn_linear_bwd: BatchNorm in front of a Linear (weight W [R, D]) whose input needs no gradient.  G holds G0 = d_pre^T x
 *                    (the Linear's weight gradient on the RAW input) and receives dW = (G0 - db mean^T) diag(rstd * gamma) + db beta^T;
 *                    partial [capmi_bn_row_blocks(R)][2][D] receives per 16 rows of W the sums of W * (G0 - db mean^T) diag(rstd)
 *                    (d gamma) and of W * db (d beta) for capmi_bn_colsum_parts.
 * The 16-byte path is used where D % 4 == 0 and the matrices are 16-byte aligned, dword accesses otherwise (D = 2053).
 * CAPMI_EINVAL, before anything is launched: a NULL required pointer, rows / D / R <= 0, more than 65535 row blocks, a float pointer
 * off 4 bytes, num_batches_tracked off 8.
 * ------------------------------------------------------------------------------------------- */
int capmi_bn_row_blocks(int rows);
int capmi_bn_stats(const float *x, const float *mask, int rows, int D, float *partial, void *stream);
int capmi_bn_finalize(const float *partial, const float *x, const float *mask, int rows, int D, int train, float eps, float momentum,
                      float *running_mean, float *running_var, int64_t *num_batches_tracked, float *mean, float *rstd, float *count,
                      float *shift, void *stream);
int capmi_bn_apply(const float *x, const float *mask, const float *shift, const float *rstd, const float *gamma, const float *beta,
                   float *y, int rows, int D, void *stream);
int capmi_bn_bwd_partial(const float *dy, const float *x, const float *mask, const float *mean, const float *rstd, int rows, int D,
                         float *partial, void *stream);
int capmi_bn_colsum_parts(const float *partial, int nparts, int D, float *out0, float *out1, void *stream);
int capmi_bn_bwd_dx(const float *dy, const float *x, const float *mask, const float *mean, const float *rstd, const float *gamma,
                    const float *dgamma, const float *dbeta, const float *count, int train, float *dx, int rows, int D, void *stream);
int capmi_bn_linear_bwd(float *G, const float *db, const float *W, const float *mean, const float *rstd, const float *gamma,
                        const float *beta, int R, int D, float *partial, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Per-word region attention of a decoded caption (att_trace.hip; opt['return_attention'], tools/eval.py --dump_attention).
 * One launch each, one wave per (caption row, step), no atomics, nothing waits for the device.  Weights are copied, not recomputed.
 * capmi_att_trace_rollout: alpha [T, N, K] as the rollouts keep it (step-major, K = the clipped region count) and seq [N, L]
 *          -> att [N, L, Kout], caption-major.  Kept steps are those where losses._shifted_mask is 1: step 0 and every step
 *          l < T whose previous token seq[n, l - 1] is not 0 (the EOS step is kept); every other step, and every column behind
 *          the source's, is WRITTEN as 0 (no memset needed; alpha is not read there, so steps an early exit left unwritten are
 *          harmless).  beta (optional, [T, N]): a weight with a column of its own in front of the regions -- column 0 = beta,
 *          columns 1 .. K = alpha.  (AdaAtt keeps its sentinel weight as column 0 of pi [T, N, K + 1], which is passed as alpha with
 *          K + 1 columns and no beta.)  T <= L is the number of steps alpha holds.
 * capmi_att_trace_beam: alpha_rows [L, rows_src, K] by SEARCH row and step, lineage [L, rows] and
 *          length [rows] of capmi_beam_finalize -> att [rows, L, Kout]: att[i, l] = alpha_rows[l, lineage[l, i]] for l < length[i]
 *          (and a lineage inside [0, rows_src)), 0 elsewhere.
 * capmi_att_ground: att [N, L, Kw] -> per (row, step) top (int32: the arg-max column, the lowest index among equal weights, -1 on a
 *          step without a positive weight), top_w (its weight, 0 there), entropy (-sum a ln a in float32, 0 ln 0 = 0).
 *          att must be finite (every producer above writes finite weights or 0): a NaN compares false with everything, so a row that
 *          holds one could be reported as a zeroed step.
 *          boxes [B, Kb, 4] with box [N, L, 4] (both or neither; 16-byte aligned): box = sum_k att[.., col0 + k] * boxes[r / n, k]
 *          for caption row r; col0 is the number of leading columns without a box (1 for AdaAtt's sentinel column, else 0).
 * CAPMI_EINVAL, before anything is launched: a NULL required pointer, a dimension <= 0, T > L, more source columns than Kout,
 *          N * L (rows * L) above 2^31 - 1, a pointer off its element size, boxes without box or the reverse, B * n < N,
 *          col0 + Kb > Kw, boxes / box off 16 bytes.
 * ------------------------------------------------------------------------------------------- */
int capmi_att_trace_rollout(const float *alpha, const float *beta, const int64_t *seq, int T, int N, int L, int K, int Kout,
                            float *att, void *stream);
int capmi_att_trace_beam(const float *alpha_rows, const int32_t *lineage, const int32_t *length, int L, int rows_src, int rows, int K,
                         int Kout, float *att, void *stream);
int capmi_att_ground(const float *att, int N, int L, int Kw, const float *boxes, int B, int n, int col0, int Kb, int32_t *top,
                     float *top_w, float *entropy, float *box, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Stochastic beam search (sbs.hip; opt['sample_method'] = 'sbs', beam.stochastic_beam_search_steps): sample_n DISTINCT captions per
 * image, drawn without replacement from the model (Kool, van Hoof and Welling 2019).  Every hypothesis carries its joint log-prob
 * phi and a perturbed value g; a step keeps the bd children with the largest perturbed values.
 * capmi_sbs_select: one step.  logp [B * cur, V1] normalised rows, image-major as in capmi_beam_select; phi / g / alive [B, cur]
 *          (alive uint8: 0 = the hypothesis has ended); noise either gumbel [B * cur, V1] (injected) or, gumbel == NULL, standard
 *          Gumbel variates from Philox (seed, offset = the step; the stream follows capmi_rng_bind_epoch like every seeded kernel).
 *          Per row j of an image: s_v = phi_j + logp[j, v] + G_v, Z_j = max_v s_v.  step0 (cur = 1, the root): the candidate's
 *          value is s_v.  Otherwise u = g_j - s_v + log(1 - exp(s_v - Z_j)), value = g_j - max(0, u) - log1p(exp(-|u|)) -- the
 *          children's values conditioned on their maximum being g_j -- and exactly g_j at the arg-max.  A row that is not alive has
 *          one candidate: token 0, phi_j, g_j bit for bit.  -inf entries of logp are never candidates.
 *          Outputs [B, bd], by descending value, equal values by the lower flat index row * V1 + token: parent (the row j), token,
 *          phi_out = phi_j + logp[j, token], g_out, alive_out = the parent was alive, token != 0 and !force_end.  An image with
 *          fewer than bd candidates fills the rest with parent 0, token 0, phi / g -inf, alive 0.
 *          scratch: capmi_sbs_scratch_bytes(B, cur, bd, V1) bytes, 4-byte aligned (the per-chunk candidate lists).
 *          Two launches, no atomics, bit-identical from run to run.  CAPMI_EINVAL, before anything is launched: a NULL pointer
 *          (gumbel excepted), a dimension <= 0, cur > bd, bd > 16, cur * V1 < bd, step0 with cur != 1, a scratch that is too small,
 *          ceil(V1 / 1024) * bd above 6144.
 * capmi_sbs_backtrack: the [L][B, bd] tables parent / token / alive_out of L steps (the last one with force_end) ->
 *          seq [B * bd, L] (0 behind the end), length [B * bd] (the end token's step counts) and lineage [L][B * bd] with the
 *          conventions of capmi_beam_finalize (capmi_lineage_gather and capmi_att_trace_beam read it as they read that one's).
 * ------------------------------------------------------------------------------------------- */
int64_t capmi_sbs_scratch_bytes(int B, int cur, int bd, int V1);
int capmi_sbs_select(const float *logp, const float *phi, const float *g, const uint8_t *alive, const float *gumbel,
                     uint64_t seed, uint32_t offset, int B, int cur, int bd, int V1, int step0, int force_end, void *scratch,
                     int64_t scratch_bytes, int32_t *parent, int64_t *token, float *phi_out, float *g_out, uint8_t *alive_out,
                     void *stream);
int capmi_sbs_backtrack(const int32_t *parent, const int64_t *token, const uint8_t *alive, int B, int bd, int L, int64_t *seq,
                        int32_t *length, int32_t *lineage, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Constrained beam search (cbs.hip; opt['constraints'], beam.constrained_beam_search_steps): captions that must contain given
 * words (Anderson, Fernando, Johnson and Gould 2017).  An image has C <= 4 constraints, each a set of <= 8 token ids that is
 * satisfied once one of them is emitted; a hypothesis's state is the bitmask of its satisfied constraints, and the image keeps one
 * beam of b slots per state: S = 2^C states (of the batch's largest C), slot = state * b + j, S * b <= 64.
 * capmi_cbs_select: one step.  logp [B * cur, V1] rows, image-major (cur = 1: the root, in state 0; else cur = S * b, row = slot);
 *          sums [B, S * b], a value that is not > -inf marks an empty slot, which is never a source whatever its row holds;
 *          words [B, 4, 8] int32 padded with -1, ncons [B] int32.  sat(v) = the mask of every constraint c < ncons whose set holds
 *          v.  The candidates of target state s' are all (valid source slot r in state s, token v) with s | sat(v) == s' and a
 *          score = sums[r] + logp[r, v] (one float32 add) > -inf.  Outputs [B, S * b]: per target state its b best by descending
 *          score, equal scores by the lower flat index r * V1 + v: parent (r), token, score, ended = token == 0 or force_end,
 *          next_sums = ended ? score - 1000 : score, valid = 1; a state with fewer candidates fills its other slots with
 *          parent 0, token 0, score / next_sums -inf, ended 0, valid 0.  With S = 1 this is capmi_beam_select bit for bit.
 *          scratch: capmi_cbs_scratch_bytes(B, cur, b, V1) bytes, 4-byte aligned (the per-chunk candidate lists).
 *          Two launches, no float atomics, bit-identical from run to run.  CAPMI_EINVAL, before anything is launched: a NULL
 *          pointer, a dimension <= 0, S no power of two <= 16, S * b > 64, cur not in {1, S * b}, a scratch that is too small,
 *          ceil((V1 + 3) / 1024) * b above 2048.  The tables are trusted to hold ids in [1, V1) and 2^ncons <= S (ops.cbs_tables
 *          checks them on the host before they are uploaded); an entry outside is skipped, a larger ncons is cut.
 * capmi_cbs_finalize: the [L][B, S * b] tables of L steps (the last one with force_end) -> per image the best recorded (ended
 *          and valid) candidate by (a) its state being the image's full mask 2^ncons - 1, else the larger popcount of the state,
 *          (b) the larger (double)score / len_div[t] (len_div NULL: the score), (c) the lower step, then the lower slot; seq [B, L]
 *          (0 behind the end), lineage [L][B] and length [B] with the conventions of capmi_beam_finalize (rows_src = S * b per
 *          image), state [B] the candidate's mask, score_out [B] its key (b).  One launch.  CAPMI_EINVAL: a NULL pointer
 *          (len_div excepted), the shape rules above, L * S * b > 4096.
 * ------------------------------------------------------------------------------------------- */
int64_t capmi_cbs_scratch_bytes(int B, int cur, int b, int V1);
int capmi_cbs_select(const float *logp, const float *sums, const int32_t *words, const int32_t *ncons, int B, int cur, int b, int S,
                     int V1, int force_end, void *scratch, int64_t scratch_bytes, int32_t *parent, int64_t *token, float *score,
                     float *next_sums, uint8_t *ended, uint8_t *valid, void *stream);
int capmi_cbs_finalize(const int32_t *parent, const int64_t *token, const float *score, const uint8_t *ended, const uint8_t *valid,
                       const int32_t *ncons, const double *len_div, int B, int b, int S, int L, int64_t *seq, int32_t *lineage,
                       int32_t *length, int32_t *state, float *score_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring given captions (score.hip; score.score_captions, model(..., mode='score'), tools/eval.py --self_retrieval /
 * --score_json): log p(caption | image) of captions that came from elsewhere, one decoder row per (image, caption) pair.
 * capmi_score_step: one step.  logits [rows, ld] (ld >= V1 floats between rows; neither ld nor V1 need be a multiple of 4), tok
 *          int64 [rows] the row's given token, live uint8 [rows].  For every row with live != 0:
 *              lse = logsumexp_v(logits[row, v] * inv_temperature) over all V1 columns,
 *              lp  = logits[row, tok] * inv_temperature - lse, 1000 lower when tok == unk_col (capmi_beam_logsoftmax's
 *                    suppress_UNK: the row is normalised over every column, then that column is pushed down; -1: none),
 *              acc[row] += lp, cnt[row] += 1, tok_logp[row] = lp (tok_logp may be NULL), and live[row] = 0 when tok == 0: the end
 *              token is scored, then the row is dead.
 *          Rows with live == 0 are not read and nothing of theirs is written.  One pass over the row (an online max / sum), 16-byte
 *          loads between the row's own 16-byte boundaries; a wave per row up to 1024 columns, a workgroup per row above; fixed
 *          reduction order, bit-identical from run to run.  Reads rows * V1 * 4 bytes, writes O(rows).  A token outside [0, V1) is
 *          the caller's error (score.py checks the captions on the host, once per call): such a row reads no logit and gets NaN.
 *          CAPMI_EINVAL, before anything is launched: a NULL pointer (tok_logp excepted), rows <= 0, V1 <= 0, ld < V1,
 *          inv_temperature not in (0, inf).
 * capmi_retrieval_rank: S [C, ld] (ld >= I), S[c, i] the score of caption c against image i of a pool, target int32 [C] the
 *          caption's own image t.  rank[c] = 1 + #{i : S[c, i] > S[c, t]} + #{i < t : S[c, i] == S[c, t]} (ties go to the lower
 *          image index), log_post[c] (may be NULL) = S[c, t] - logsumexp_i S[c, i], the posterior of the right image under a
 *          uniform prior.  One workgroup per caption.  A target outside [0, I) (ops.retrieval_rank refuses it) gives rank 0 and
 *          NaN.  CAPMI_EINVAL: a NULL pointer (log_post excepted), C <= 0, I <= 0, ld < I.
 * ------------------------------------------------------------------------------------------- */
int capmi_score_step(const float *logits, int64_t ld, int rows, int V1, const int64_t *tok, uint8_t *live, float *acc, int32_t *cnt,
                     float *tok_logp, float inv_temperature, int unk_col, void *stream);
int capmi_retrieval_rank(const float *S, int64_t ld, int C, int I, const int32_t *target, int32_t *rank, float *log_post,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CAPMI_H */
