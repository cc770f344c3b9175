// NewFC decoder on gfx950: maxout-LSTM cell kernels + whole-rollout drivers (forward and BPTT).
// Replaces NewFCModel.core / _prepare_feature (AttModel.py:904-945) over LSTMCore (FCModel.py:13-42)
// and the time loops of AttModel._forward / _sample for that model.  One host call per rollout, no host
// sync, time-batched weight gradients; the driver plumbing around the step is rollout_common.h's.
// The cell kernels also serve Att2in2 (att2in2.hip), whose cell is this one with an a2c term on the candidate half:
// capmi_att2in2_cell_fwd / _bwd are defined here beside capmi_maxout_cell_fwd / _bwd.
#include "rollout_common.h"

using namespace capmi;

namespace {

// sum_s p[s * slab + off] over the K-slice slabs of a GEMM, four independent loads at a time
__device__ __forceinline__ float slab_sum(const float *__restrict__ p, int splits, size_t slab, size_t off) {
    float v = 0.f;
    for (int k0 = 0; k0 < splits; k0 += 4) {
        float tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tv[u] = (k0 + u < splits) ? p[(size_t)(k0 + u) * slab + off] : 0.f;
        v += tv[0] + tv[1] + tv[2] + tv[3];
    }
    return v;
}

// sums[r, q*R + j] = sum_s partial[s][r][q*R + j] (+ addend) + b_i2h + b_h2h; Att2in2 (partial2 or b_a2c given) adds to the
// candidate half, q = 3, 4: sum_s partial2[s][r][(q-3)*R + j] + b_a2c.  saved = (sig(in), sig(f), sig(out), cand_a, cand_b).
__global__ void maxout_cell_fwd_kernel(const float *__restrict__ partial, int splits, const float *__restrict__ partial2,
                                       int splits2, const float *__restrict__ addend, const float *__restrict__ b_i2h,
                                       const float *__restrict__ b_h2h, const float *__restrict__ b_a2c,
                                       const float *__restrict__ c_prev, float *__restrict__ h, float *__restrict__ c,
                                       float *__restrict__ saved, const float *__restrict__ out_mask,
                                       float *__restrict__ h_drop, int N, int R) {
    const size_t total = (size_t)N * R, slab = (size_t)N * 5 * R, slab2 = (size_t)N * 2 * R;
    const bool a2c = partial2 || b_a2c;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / R), j = (int)(i % R);
        float s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const size_t col = (size_t)q * R + j;
            float v = slab_sum(partial, splits, slab, (size_t)r * 5 * R + col);
            if (addend) v += addend[(size_t)r * 5 * R + col];
            if (b_i2h) v += b_i2h[col];
            if (b_h2h) v += b_h2h[col];
            if (q >= 3 && a2c) {
                const size_t col2 = (size_t)(q - 3) * R + j;
                float a = slab_sum(partial2, splits2, slab2, (size_t)r * 2 * R + col2);
                if (b_a2c) a += b_a2c[col2];
                v += a;
            }
            s[q] = v;
        }
        const float ig = sigmoid_f(s[0]), fg = sigmoid_f(s[1]), og = sigmoid_f(s[2]);
        const float cand = fmaxf(s[3], s[4]);
        const float cn = fg * c_prev[i] + ig * cand;
        const float hn = og * tanh_f(cn);
        c[i] = cn;
        h[i] = hn;
        float *sv = saved + (size_t)r * 5 * R + j;
        sv[0] = ig; sv[R] = fg; sv[2 * R] = og; sv[3 * (size_t)R] = s[3]; sv[4 * (size_t)R] = s[4];
        if (h_drop) h_drop[i] = out_mask ? hn * out_mask[i] : hn;
    }
}

// dh = dh_a (* dh_a_mask) + sum_s dh_b[s * b_stride + i] (the dX GEMM of the step after as K-slice slabs, or one finished buffer:
// b_splits = 1); d_sums [N,5R], dc_prev.
__global__ void maxout_cell_bwd_kernel(const float *__restrict__ dh_a, const float *__restrict__ dh_a_mask,
                                       const float *__restrict__ dh_b, int b_splits, int64_t b_stride,
                                       const float *__restrict__ dc_next, const float *__restrict__ saved,
                                       const float *__restrict__ c_prev, const float *__restrict__ c_new,
                                       float *__restrict__ d_sums, float *__restrict__ dc_prev, int N, int R) {
    const size_t total = (size_t)N * R;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / R), j = (int)(i % R);
        float dh = 0.f;
        if (dh_a) dh += dh_a_mask ? dh_a[i] * dh_a_mask[i] : dh_a[i];
        if (dh_b)
            for (int k = 0; k < b_splits; ++k) dh += dh_b[(size_t)k * b_stride + i];
        const float *sv = saved + (size_t)r * 5 * R + j;
        const float ig = sv[0], fg = sv[R], og = sv[2 * R], ca = sv[3 * (size_t)R], cb = sv[4 * (size_t)R];
        const float cand = fmaxf(ca, cb);
        const float tc = tanh_f(c_new[i]);
        float dc = dh * og * (1.f - tc * tc);
        if (dc_next) dc += dc_next[i];
        float *ds = d_sums + (size_t)r * 5 * R + j;
        ds[0] = dc * cand * ig * (1.f - ig);
        ds[R] = dc * c_prev[i] * fg * (1.f - fg);
        ds[2 * R] = dh * tc * og * (1.f - og);
        const float dcand = dc * ig;
        ds[3 * (size_t)R] = ca >= cb ? dcand : 0.f;       // torch.max(a, b) routes the gradient to the larger chunk
        ds[4 * (size_t)R] = ca >= cb ? 0.f : dcand;
        dc_prev[i] = dc * fg;
    }
}

}  // namespace

extern "C" {

int capmi_att2in2_cell_fwd(const float *partial, int splits, const float *partial2, int splits2, const float *addend,
                           const float *b_i2h, const float *b_h2h, const float *b_a2c, const float *c_prev, float *h, float *c,
                           float *saved, const float *out_mask, float *h_drop, int N, int R, void *stream) {
    if (!partial || splits < 1 || splits2 < 0 || (splits2 > 0 && !partial2) || !c_prev || !h || !c || !saved || N <= 0 || R <= 0)
        return CAPMI_EINVAL;
    hipLaunchKernelGGL(maxout_cell_fwd_kernel, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, partial,
                       splits, partial2, splits2, addend, b_i2h, b_h2h, b_a2c, c_prev, h, c, saved, out_mask, h_drop, N, R);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_att2in2_cell_bwd(const float *dh_a, const float *dh_a_mask, const float *dh_b, int b_splits, int64_t b_stride,
                           const float *dc_next, const float *saved, const float *c_prev, const float *c_new, float *d_sums,
                           float *dc_prev, int N, int R, void *stream) {
    if (!saved || !c_prev || !c_new || !d_sums || !dc_prev || N <= 0 || R <= 0 || (dh_b && (b_splits < 1 || b_stride < (int64_t)N * R)))
        return CAPMI_EINVAL;
    hipLaunchKernelGGL(maxout_cell_bwd_kernel, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, dh_a,
                       dh_a_mask, dh_b, b_splits, b_stride, dc_next, saved, c_prev, c_new, d_sums, dc_prev, N, R);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_maxout_cell_fwd(const float *partial, int splits, const float *b_i2h, const float *b_h2h, const float *c_prev,
                          float *h, float *c, float *saved, const float *out_mask, float *h_drop, int N, int R,
                          void *stream) {
    return capmi_att2in2_cell_fwd(partial, splits, nullptr, 0, nullptr, b_i2h, b_h2h, nullptr, c_prev, h, c, saved, out_mask,
                                  h_drop, N, R, stream);
}

int capmi_maxout_cell_bwd(const float *dh_a, const float *dh_a_mask, const float *dh_b, const float *dc_next,
                          const float *saved, const float *c_prev, const float *c_new, float *d_sums, float *dc_prev,
                          int N, int R, void *stream) {
    return capmi_att2in2_cell_bwd(dh_a, dh_a_mask, dh_b, 1, (int64_t)N * R, dc_next, saved, c_prev, c_new, d_sums, dc_prev, N,
                                  R, stream);
}

int capmi_newfc_rollout_fwd(const capmi_newfc_weights *w, capmi_newfc_rollout *r, void *stream) {
    if (!w || !r) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, R = r->R, E = r->E, V1 = r->V1, T = r->T;
    if (B <= 0 || n <= 0 || N != B * n || !r->partial) return CAPMI_EINVAL;
    // (r5: mode may carry CAPMI_SELECT_RAW -- a free-running rollout that stores the LOGITS, AttModel._sample(output_logsoftmax=0))
    const SelectIO io = select_io(r);
    RC(check_rollout_io(io));
    const size_t NR = (size_t)N * R;
    const bool sched = scheduled(io);
    // plain Embedding: no ReLU, no mask; only scheduled sampling folds it into the select (free-running steps embed below)
    const EmbedSpec emb{w->embed, E, 0, nullptr, r->x, false};
    float *slabs = r->partial + CAPMI_WS_COUNTER_FLOATS;
    RC(capmi_rollout_init(r->h, r->c, nullptr, nullptr, (int64_t)NR, r->it, r->unfinished, N, stream));    // state 0, BOS
    int splits = 1;
    // step "-1": the image (AttModel.py:925-927); h = c = 0 so only the i2h term matters but keep the general form.  (Its own, like
    // the per-step embed below: no select and a row divisor; teacher_inputs would embed all steps first and reorder the launches.)
    {
        SegSpec s[2] = {{r->fc_emb, E, w->i2h_w, E, E, n}, {r->h, R, w->h2h_w, R, R, 1}};
        RC(gemm(stream, 0, 0, N, 5 * R, r->partial, 5 * R, s, 2, r->partial, r->partial_capacity, 1, &splits));
        RC(capmi_maxout_cell_fwd(slabs, splits, w->i2h_b, w->h2h_b, r->c, r->h + NR, r->c + NR, r->saved, nullptr, nullptr, N,
                                 R, stream));
    }
    for (int t = 0; t < T; ++t) {
        float *x = r->x + (size_t)t * N * E;
        const float *h_prev = r->h + (size_t)(t + 1) * NR, *c_prev = r->c + (size_t)(t + 1) * NR;
        float *h = r->h + (size_t)(t + 2) * NR, *c = r->c + (size_t)(t + 2) * NR;
        float *h_drop = r->h_drop + (size_t)t * NR;
        if (sched && t > 0) {
            // scheduled sampling: x[t] and it_all[t] were written by the select launch of step t-1
        } else if (r->teacher)
            RC(capmi_embed_fwd(r->forced + t, r->forced_ld, r->it_all + (size_t)t * N, w->embed, nullptr, x, N, E, 0, stream));
        else
            RC(capmi_embed_fwd(r->it, 1, r->it_all + (size_t)t * N, w->embed, nullptr, x, N, E, 0, stream));
        SegSpec s[2] = {{x, E, w->i2h_w, E, E, 1}, {h_prev, R, w->h2h_w, R, R, 1}};
        RC(gemm(stream, 0, 0, N, 5 * R, r->partial, 5 * R, s, 2, r->partial, r->partial_capacity, 1, &splits));
        RC(capmi_maxout_cell_fwd(slabs, splits, w->i2h_b, w->h2h_b, c_prev, h, c, r->saved + (size_t)(t + 1) * N * 5 * R,
                                 r->drop_out ? r->drop_out + (size_t)t * NR : nullptr, h_drop, N, R, stream));
        RC(logit_slabs(stream, h_drop, w->logit_w, N, V1, R, r->partial, r->partial_capacity, &splits));
        RC(select_step(io, t, slabs, splits, w->logit_b, emb, stream));
    }
    return 0;
}

int capmi_newfc_rollout_bwd(const capmi_newfc_weights *w, const capmi_newfc_rollout *r, const float *g_seq_logp,
                            capmi_newfc_bwd_scratch *s, capmi_newfc_grads *g, void *stream) {
    if (!w || !r || (!g_seq_logp && !(s && s->sparse)) || !s || !g) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, R = r->R, E = r->E, V1 = r->V1, T = r->T;
    hipStream_t st = (hipStream_t)stream;
    const size_t NR = (size_t)N * R;
    const int TN = T * N;
    float *P = s->partial;
    const int64_t cap = s->partial_capacity;
    RC(logit_bwd_head(select_io(r), s->sparse, g_seq_logp, s->dlogits, w->logit_w, R, s->d_hdrop, P, cap, stream));
    static const int env_group = capmi::knob("CAPMI_GEMM_GROUP", 1);
    const bool grouped = env_group != 0;
    capmi_group_gemm grp[3];
    int n_grp = 0;
    {
        // r6: the three time-batched weight gradients (logit, i2h, h2h: K = T * N rows -- 1 050 at bs10 x 5, not a multiple of 4, which
        // sent them to the exact-fp32 tile kernel: 263 us of a 1.9-ms step) are listed and go out as ONE grouped launch at the end;
        // the logit bias gradient rides in it.  CAPMI_GEMM_GROUP=0: one launch each, as before.  (Not grouped_dw_with_bias: the
        // bias's own column sum goes out HERE, before BPTT, and the listing is interleaved with that route.)
        if (grouped) {
            grp[n_grp++] = capmi_group_gemm{s->dlogits, r->h_drop, g->logit_w, V1, R, R, TN, V1, R, 0, 0,
                                            aligned16(g->logit_b) ? g->logit_b : nullptr};
            if (!grp[n_grp - 1].colsum) RC(capmi_colsum(s->dlogits, TN, V1, V1, g->logit_b, 0, stream));
        } else {
            SegSpec b{s->dlogits, V1, r->h_drop, R, TN, 1};
            RC(gemm(stream, 1, 1, V1, R, g->logit_w, R, &b, 1, P, cap, 0, nullptr));
            RC(capmi_colsum(s->dlogits, TN, V1, V1, g->logit_b, 0, stream));
        }
    }
    for (int t = T - 1; t >= -1; --t) {
        const int slot = t + 1;                       // saved / d_sums slot (0 = image step)
        float *d_sums = s->d_sums + (size_t)slot * N * 5 * R;
        RC(capmi_maxout_cell_bwd(t >= 0 ? s->d_hdrop + (size_t)t * NR : nullptr,
                                 (t >= 0 && r->drop_out) ? r->drop_out + (size_t)t * NR : nullptr, pp_in(s->dh_prev, t, T, NR),
                                 pp_in(s->dc, t, T, NR), r->saved + (size_t)slot * N * 5 * R, r->c + (size_t)slot * NR,
                                 r->c + (size_t)(slot + 1) * NR, d_sums, pp_out(s->dc, t, NR), N, R, stream));
        if (t >= 0) {   // dh_prev = d_sums W_h2h (the image step's predecessor state is the constant zero)
            SegSpec a{d_sums, 5 * R, w->h2h_w, R, 5 * R, 1};
            RC(gemm(stream, 0, 1, N, R, pp_out(s->dh_prev, t, NR), R, &a, 1, P, cap, 0, nullptr));
        }
    }
    // time-batched gradients.  d_sums slots 1..T belong to the word steps, slot 0 to the image step.
    const float *ds_words = s->d_sums + (size_t)N * 5 * R;
    {
        SegSpec a{ds_words, 5 * R, r->x, E, TN, 1};                       // dW_i2h (words)
        if (!grouped) RC(gemm(stream, 1, 1, 5 * R, E, g->i2h_w, E, &a, 1, P, cap, 0, nullptr));
        // + image step: x = fc_emb[row / n] is shared by the n rows of an image, so their d_sums are summed first (d_x_all reused
        // as [B,5R]) and the product has K = B rows
        // (grouped: the image step WRITES the gradient here and the words' product is added to it by the grouped launch)
        RC(capmi_group_rowsum(s->d_sums, 1, 0, B, n, 5 * R, s->d_x_all /* reuse as [B,5R] sum */, stream));
        SegSpec img{s->d_x_all, 5 * R, r->fc_emb, E, B, 1};
        RC(gemm(stream, 1, 1, 5 * R, E, g->i2h_w, E, &img, 1, P, cap, 0, nullptr, nullptr, nullptr, grouped ? 0 : 1));
        // d_fc_emb [B,E] = (sum over the n rows of the image of d_sums_img) W_i2h
        if (g->d_fc_emb) {
            SegSpec f{s->d_x_all, 5 * R, w->i2h_w, E, 5 * R, 1};
            RC(gemm(stream, 0, 1, B, E, g->d_fc_emb, E, &f, 1, P, cap, 0, nullptr));
        }
        // bias gradients: all T+1 steps
        RC(capmi_colsum(s->d_sums, (T + 1) * N, 5 * R, 5 * R, g->i2h_b, 0, stream));
        HIP_RC(hipMemcpyAsync(g->h2h_b, g->i2h_b, (size_t)5 * R * sizeof(float), hipMemcpyDeviceToDevice, st));
        // dW_h2h: h_prev of word step t is slot t+1; of the image step it is slot 0 (zeros) -> words only
        SegSpec c{ds_words, 5 * R, r->h + NR, R, TN, 1};
        if (grouped) {
            grp[n_grp++] = capmi_group_gemm{ds_words, r->x, g->i2h_w, 5 * R, E, E, TN, 5 * R, E, 1, 0, nullptr};
            grp[n_grp++] = capmi_group_gemm{ds_words, r->h + NR, g->h2h_w, 5 * R, R, R, TN, 5 * R, R, 0, 0, nullptr};
        } else RC(gemm(stream, 1, 1, 5 * R, R, g->h2h_w, R, &c, 1, P, cap, 0, nullptr));
        // word embeddings (plain Embedding: no ReLU, no dropout)
        RC(embed_grad(stream, SegSpec{ds_words, 5 * R, w->i2h_w, E, 5 * R, 1}, TN, E, s->d_x_all, r->it_all, nullptr, nullptr, 0,
                      g->embed, V1, P, cap));
    }
    if (n_grp) RC(capmi_gemm_group_tn(grp, n_grp, cap > CAPMI_WS_COUNTER_FLOATS ? P + CAPMI_WS_COUNTER_FLOATS : nullptr,
                                      cap > CAPMI_WS_COUNTER_FLOATS ? cap - CAPMI_WS_COUNTER_FLOATS : 0, stream));
    return 0;
}

}  // extern "C"
