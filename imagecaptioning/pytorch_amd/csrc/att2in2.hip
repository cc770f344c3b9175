// Att2in2 decoder on gfx950: whole-rollout drivers (forward and BPTT) and a single decode step.
// Replaces Att2in2Core.forward (AttModel.py:750-790) under Att2in2Model (AttModel.py:854-859) and the time loops of
// AttModel._forward / _sample for that model.  The recurrence is the NewFC maxout cell whose candidate half also receives
// a2c(att_res): capmi_att2in2_cell_fwd / _bwd, defined with the NewFC cell kernels in newfc.hip.  The attention is UpDown's
// additive region attention (attention.hip), queried with the state BEFORE the step.  One host call per rollout, no host sync,
// time-batched weight gradients as one grouped launch; the driver plumbing around the step is rollout_common.h's.
#include "rollout_common.h"

using namespace capmi;

namespace {

// One recurrent step without the vocabulary projection: h2att of h_prev -> attention -> gates (x . i2h + h_prev . h2h, or the
// h2h half only when the i2h product of the step is given as `xin`) -> a2c(ctx) -> cell.
int core_step(const capmi_att2in2_weights *w, const Carve &ws, int B, int n, int N, int K, int A, int R, int E,
              const float *att, const float *p_att, const float *att_mask, const float *x, const float *xin,
              const float *h_prev, const float *c_prev, float *att_h, float *alpha, float *ctx, float *h, float *c, float *saved,
              const float *out_mask, float *h_drop, void *stream) {
    float *slabs1 = ws.p1 + CAPMI_WS_COUNTER_FLOATS, *slabs2 = ws.p2 + CAPMI_WS_COUNTER_FLOATS;
    int splits = 1, splits2 = 1;
    {
        SegSpec s{h_prev, R, w->h2att_w, R, R};
        RC(gemm(stream, 0, 0, N, A, ws.p1, A, &s, 1, ws.p1, ws.cap1, 1, &splits));
    }
    RC(capmi_attention_fwd_partial(slabs1, splits, (int64_t)N * A, w->h2att_b, att_h, p_att, att, att_mask, w->alpha_w,
                                   w->alpha_b, ctx, alpha, B, n, K, A, R, nullptr, N, stream));
    if (xin) {
        SegSpec s{h_prev, R, w->h2h_w, R, R};
        RC(gemm(stream, 0, 0, N, 5 * R, ws.p1, 5 * R, &s, 1, ws.p1, ws.cap1, 1, &splits));
    } else {
        SegSpec s[2] = {{x, E, w->i2h_w, E, E}, {h_prev, R, w->h2h_w, R, R}};
        RC(gemm(stream, 0, 0, N, 5 * R, ws.p1, 5 * R, s, 2, ws.p1, ws.cap1, 1, &splits));
    }
    {
        SegSpec s{ctx, R, w->a2c_w, R, R};
        RC(gemm(stream, 0, 0, N, 2 * R, ws.p2, 2 * R, &s, 1, ws.p2, ws.cap2, 1, &splits2));
    }
    return capmi_att2in2_cell_fwd(slabs1, splits, slabs2, splits2, xin, w->i2h_b, w->h2h_b, w->a2c_b, c_prev, h, c, saved,
                                  out_mask, h_drop, N, R, stream);
}

}  // namespace

extern "C" {

int capmi_att2in2_rollout_fwd(const capmi_att2in2_weights *w, capmi_att2in2_rollout *r, void *stream) {
    if (!w || !r) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, K = r->K, A = r->A, R = r->R, E = r->E, V1 = r->V1, T = r->T;
    if (B <= 0 || n <= 0 || N != B * n || K <= 0 || A <= 0 || !r->partial || !r->att || !r->p_att) return CAPMI_EINVAL;
    const SelectIO io = select_io(r);
    RC(check_rollout_io(io));
    Carve ws;
    if (!carve(r->partial, r->partial_capacity, &ws)) return CAPMI_EINVAL;
    const size_t NR = (size_t)N * R;
    // teacher forcing knows every input token up front: the i2h half of the gates of all T steps is ONE GEMM over T*N rows
    const bool batched_x = r->teacher && !scheduled(io) && r->xin;
    const EmbedSpec emb{w->embed, E, 1, r->drop_xt, r->x, true};
    RC(capmi_rollout_init(r->h, r->c, nullptr, nullptr, (int64_t)NR, r->it, r->unfinished, N, stream));    // state 0, BOS
    RC(teacher_inputs(io, emb, w->i2h_w, 5 * R, batched_x ? r->xin : nullptr, ws.p1, ws.cap1, stream));
    for (int t = 0; t < T; ++t) {
        const float *x = r->x + (size_t)t * N * E;
        float *h_drop = r->h_drop + (size_t)t * NR;
        RC(core_step(w, ws, B, n, N, K, A, R, E, r->att, r->p_att, r->att_mask, x, batched_x ? r->xin + (size_t)t * N * 5 * R : nullptr,
                     r->h + (size_t)t * NR, r->c + (size_t)t * NR, r->att_h + (size_t)t * N * A, r->alpha + (size_t)t * N * K,
                     r->ctx + (size_t)t * NR, r->h + (size_t)(t + 1) * NR, r->c + (size_t)(t + 1) * NR,
                     r->saved + (size_t)t * N * 5 * R, r->drop_out ? r->drop_out + (size_t)t * NR : nullptr, h_drop, stream));
        int splits = 1;
        RC(logit_slabs(stream, h_drop, w->logit_w, N, V1, R, ws.p1, ws.cap1, &splits));
        RC(select_step(io, t, ws.p1 + CAPMI_WS_COUNTER_FLOATS, splits, w->logit_b, emb, stream));
    }
    return 0;
}

int capmi_att2in2_rollout_bwd(const capmi_att2in2_weights *w, const capmi_att2in2_rollout *r, const float *g_seq_logp,
                              capmi_att2in2_bwd_scratch *s, capmi_att2in2_grads *g, void *stream) {
    if (!w || !r || (!g_seq_logp && !(s && s->sparse)) || !s || !g) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, K = r->K, A = r->A, R = r->R, E = r->E, V1 = r->V1, T = r->T;
    if (!s->partial || s->partial_capacity <= CAPMI_WS_COUNTER_FLOATS) return CAPMI_EINVAL;
    const size_t NR = (size_t)N * R;
    const int TN = T * N;
    float *P = s->partial;
    const int64_t cap = s->partial_capacity;
    float *slabs = P + CAPMI_WS_COUNTER_FLOATS;
    RC(logit_bwd_head(select_io(r), s->sparse, g_seq_logp, s->dlogits, w->logit_w, R, s->d_hdrop, P, cap, stream));
    // BPTT.  Per step: cell (dh = d_hdrop * mask + the previous iteration's dh slabs) -> a2c dX as slabs, finished and published by
    // the attention Jacobian (d_ctx, d_att_h, d_e) -> dh_prev = d_att_h W_h2att + d_sums W_h2h as slabs for the next cell.
    int dh_splits = 0;
    for (int t = T - 1; t >= 0; --t) {
        const bool last = (t == T - 1);
        float *d_sums = s->d_sums + (size_t)t * N * 5 * R;
        float *d_att_h = s->d_att_h + (size_t)t * N * A;
        RC(capmi_att2in2_cell_bwd(s->d_hdrop + (size_t)t * NR, r->drop_out ? r->drop_out + (size_t)t * NR : nullptr,
                                  last ? nullptr : slabs, dh_splits, (int64_t)NR, pp_in(s->dc, t, T, NR),
                                  r->saved + (size_t)t * N * 5 * R, r->c + (size_t)t * NR, r->c + (size_t)(t + 1) * NR, d_sums,
                                  pp_out(s->dc, t, NR), N, R, stream));
        int x_splits = 1;
        {
            SegSpec a{d_sums + 3 * R, 5 * R, w->a2c_w, R, 2 * R};      // d_att_res = d_sums[:, 3R:5R] W_a2c, read in place
            RC(gemm(stream, 0, 1, N, R, P, R, &a, 1, P, cap, 1, &x_splits));
        }
        RC(capmi_attention_bwd_partial(slabs, x_splits, (int64_t)NR, R, s->d_ctx + (size_t)t * NR, r->att_h + (size_t)t * N * A,
                                       r->alpha + (size_t)t * N * K, r->p_att, r->att, w->alpha_w, d_att_h,
                                       s->d_e + (size_t)t * N * K, B, n, K, A, R, nullptr, N, stream));
        if (t > 0) {       // the state before step 0 is the constant zero
            SegSpec a[2] = {{d_att_h, A, w->h2att_w, R, A}, {d_sums, 5 * R, w->h2h_w, R, 5 * R}};
            RC(gemm(stream, 0, 1, N, R, P, R, a, 2, P, cap, 1, &dh_splits));
        }
    }
    // attention parameters / features, time-batched; alpha_net's weight gradient as one partial row per (image, region)
    const int64_t dw_floats = (int64_t)B * K * A;
    float *dw_part = alpha_dw_part(P, cap, dw_floats);
    RC(capmi_attention_bwd_batched_ws(s->d_ctx, R, r->att_h, r->alpha, s->d_e, r->p_att, w->alpha_w, g->d_att, g->d_p_att,
                                      dw_part ? nullptr : g->alpha_w, g->alpha_b, T, B, n, N, K, A, R, dw_part, stream));
    if (dw_part) RC(capmi_colsum(dw_part, B * K, A, A, g->alpha_w, 0, stream));
    // token embeddings: d_x = d_sums W_i2h, scattered through ReLU / dropout
    RC(embed_grad(stream, SegSpec{s->d_sums, 5 * R, w->i2h_w, E, 5 * R}, TN, E, s->d_x, r->it_all, r->x, r->drop_xt, 1, g->embed, V1,
                  P, cap));
    // the five time-batched weight gradients (K = T*N rows) with their bias column sums as ONE grouped launch; h_prev of step t is
    // state slot t, i.e. slots 0..T-1 of h
    capmi_group_gemm grp[5] = {
        {s->dlogits, r->h_drop, g->logit_w, V1, R, R, TN, V1, R, 0, 0, nullptr},
        {s->d_sums, r->x, g->i2h_w, 5 * R, E, E, TN, 5 * R, E, 0, 0, nullptr},
        {s->d_sums, r->h, g->h2h_w, 5 * R, R, R, TN, 5 * R, R, 0, 0, nullptr},
        {s->d_sums + 3 * R, r->ctx, g->a2c_w, 5 * R, R, R, TN, 2 * R, R, 0, 0, nullptr},
        {s->d_att_h, r->h, g->h2att_w, A, R, R, TN, A, R, 0, 0, nullptr}};
    const BiasCol bias[5] = {
        {g->logit_b, s->dlogits, V1, V1}, {g->i2h_b, s->d_sums, 5 * R, 5 * R}, {g->h2h_b, s->d_sums, 5 * R, 5 * R},
        {g->a2c_b, s->d_sums + 3 * R, 5 * R, 2 * R}, {g->h2att_b, s->d_att_h, A, A}};
    return grouped_dw_with_bias(grp, 5, bias, 5, dw_floats, P, cap, stream);
}

int capmi_att2in2_decode_step(const capmi_att2in2_weights *w, capmi_att2in2_step *s, int rows, int rows_per_image,
                              const float *h_src, const float *c_src, float *h_dst, float *c_dst, void *stream) {
    if (!w || !s || rows <= 0 || rows_per_image <= 0 || rows != s->B * rows_per_image || !h_src || !c_src || !h_dst || !c_dst ||
        !s->partial || !s->it)
        return CAPMI_EINVAL;
    const int B = s->B, K = s->K, A = s->A, R = s->R, E = s->E, V1 = s->V1;
    Carve ws;
    if (!carve(s->partial, s->partial_capacity, &ws)) return CAPMI_EINVAL;
    RC(capmi_embed_fwd(s->it, 1, nullptr, w->embed, nullptr, s->xt, rows, E, 1, stream));          // eval: ReLU, no dropout
    RC(core_step(w, ws, B, rows_per_image, rows, K, A, R, E, s->att, s->p_att, s->att_mask, s->xt, nullptr, h_src, c_src, s->att_h,
                 s->alpha, s->ctx, h_dst, c_dst, s->saved, nullptr, nullptr, stream));
    return decode_logits(stream, h_dst, w->logit_w, w->logit_b, rows, V1, R, s->logits, ws.p1, ws.cap1);
}

}  // extern "C"
