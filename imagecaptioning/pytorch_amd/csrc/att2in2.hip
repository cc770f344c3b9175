// Att2in2 decoder on gfx950: whole-rollout drivers (forward and BPTT) and a single decode step.
// Replaces Att2in2Core.forward (AttModel.py:750-790) under Att2in2Model (AttModel.py:854-859) and the time loops of
// AttModel._forward / _sample for that model.  The recurrence is the NewFC maxout cell whose candidate half also receives
// a2c(att_res): capmi_att2in2_cell_fwd / _bwd, defined with the NewFC cell kernels in newfc.hip.  The attention is UpDown's
// additive region attention (attention.hip), queried with the state BEFORE the step.  Same structure as the NewFC / UpDown
// drivers: one host call per rollout, no host sync, time-batched weight gradients as one grouped launch.
#include "host_common.h"

using namespace capmi;

namespace {

// The split-K workspace in two regions: the gate GEMM's slabs (main) and the a2c GEMM's (second), which the cell reads together.
struct Carve {
    float *p1; int64_t cap1;
    float *p2; int64_t cap2;
};
inline bool carve(float *partial, int64_t cap, Carve *o) {
    const int64_t cap2 = (cap / 4) & ~(int64_t)1023;
    o->p1 = partial; o->cap1 = cap - cap2;
    o->p2 = partial + o->cap1; o->cap2 = cap2;
    return o->cap1 > CAPMI_WS_COUNTER_FLOATS && o->cap2 > CAPMI_WS_COUNTER_FLOATS;
}

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
    const int B = r->B, n = r->n, N = r->N, K = r->K, A = r->A, R = r->R, E = r->E, V1 = r->V1, T = r->T, L = r->L;
    if (B <= 0 || n <= 0 || N != B * n || K <= 0 || A <= 0 || T <= 0 || L < T || !r->partial || !r->att || !r->p_att)
        return CAPMI_EINVAL;
    if (((r->mode & 255) == 2 || r->teacher) && !r->forced) return CAPMI_EINVAL;
    if (r->ss_mode && !r->teacher) return CAPMI_EINVAL;
    Carve ws;
    if (!carve(r->partial, r->partial_capacity, &ws)) return CAPMI_EINVAL;
    const size_t NR = (size_t)N * R;
    const bool sched = r->teacher && r->ss_mode;
    // teacher forcing knows every input token up front: the i2h half of the gates of all T steps is ONE GEMM over T*N rows
    const bool batched_x = r->teacher && !sched && r->xin;
    RC(capmi_rollout_init(r->h, r->c, nullptr, nullptr, (int64_t)NR, r->it, r->unfinished, N, stream));    // state 0, BOS
    if (r->teacher && !sched) {
        for (int t = 0; t < T; ++t)
            RC(capmi_embed_fwd(r->forced + t, r->forced_ld, r->it_all + (size_t)t * N, w->embed,
                               r->drop_xt ? r->drop_xt + (size_t)t * N * E : nullptr, r->x + (size_t)t * N * E, N, E, 1, stream));
        if (batched_x) {
            SegSpec s{r->x, E, w->i2h_w, E, E};
            RC(gemm(stream, 0, 0, T * N, 5 * R, r->xin, 5 * R, &s, 1, ws.p1, ws.cap1, 0, nullptr));
        }
    } else {
        // step 0's input: BOS (free-running) or forced[:, 0] (scheduled sampling); later inputs come from the select's tail
        RC(capmi_embed_fwd(r->teacher ? r->forced : r->it, r->teacher ? r->forced_ld : 1, r->it_all, w->embed, r->drop_xt, r->x,
                           N, E, 1, stream));
    }
    for (int t = 0; t < T; ++t) {
        const float *x = r->x + (size_t)t * N * E;
        float *h_drop = r->h_drop + (size_t)t * NR;
        RC(core_step(w, ws, B, n, N, K, A, R, E, r->att, r->p_att, r->att_mask, x, batched_x ? r->xin + (size_t)t * N * 5 * R : nullptr,
                     r->h + (size_t)t * NR, r->c + (size_t)t * NR, r->att_h + (size_t)t * N * A, r->alpha + (size_t)t * N * K,
                     r->ctx + (size_t)t * NR, r->h + (size_t)(t + 1) * NR, r->c + (size_t)(t + 1) * NR,
                     r->saved + (size_t)t * N * 5 * R, r->drop_out ? r->drop_out + (size_t)t * NR : nullptr, h_drop, stream));
        int splits = 1;
        {
            SegSpec s{h_drop, R, w->logit_w, R, R};
            RC(gemm(stream, 0, 0, N, V1, ws.p1, V1, &s, 1, ws.p1, ws.cap1, 1, &splits));
        }
        const float *slabs = ws.p1 + CAPMI_WS_COUNTER_FLOATS;
        const float *gum = r->gumbel ? r->gumbel + (size_t)t * N * V1 : nullptr;
        capmi_next_embed ne{};
        if ((!r->teacher || sched) && t + 1 < T) {
            ne.E = w->embed; ne.Edim = E; ne.relu = 1;
            ne.mask = r->drop_xt ? r->drop_xt + (size_t)(t + 1) * N * E : nullptr;
            ne.x = r->x + (size_t)(t + 1) * N * E;
            ne.it_save = r->it_all + (size_t)(t + 1) * N;
        }
        if (sched && t + 1 < T) {
            // AttModel.py:145-154: the token chosen here is the INPUT of step t+1 -- forced[:, t+1] (ss_mode 2 rows) or a
            // categorical draw from this step's log-probs (ss_mode 1 rows); the same launch embeds it
            RC(capmi_logsoftmax_select_partial(slabs, splits, (int64_t)N * V1, w->logit_b, N, V1, t, L, 2,
                                               r->ss_mode + (size_t)(t + 1) * N, 1.f, gum, r->seed, r->forced + 1, r->forced_ld, 1,
                                               r->seq, L, r->it, r->unfinished, r->seq_logp, r->sel_logp, r->live, &ne, nullptr,
                                               stream));
            continue;
        }
        RC(capmi_logsoftmax_select_partial(slabs, splits, (int64_t)N * V1, w->logit_b, N, V1, t, L, r->teacher ? 2 : r->mode, nullptr,
                                           r->temperature, gum, r->seed, r->forced, r->forced_ld, r->teacher ? 1 : 0, r->seq, L,
                                           r->it, r->unfinished, r->seq_logp, r->sel_logp, r->live, ne.x ? &ne : nullptr, nullptr,
                                           stream));
    }
    return 0;
}

int capmi_att2in2_rollout_bwd(const capmi_att2in2_weights *w, const capmi_att2in2_rollout *r, const float *g_seq_logp,
                              capmi_att2in2_bwd_scratch *s, capmi_att2in2_grads *g, void *stream) {
    if (!w || !r || (!g_seq_logp && !(s && s->sparse)) || !s || !g) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, K = r->K, A = r->A, R = r->R, E = r->E, V1 = r->V1, T = r->T, L = r->L;
    if (!s->partial || s->partial_capacity <= CAPMI_WS_COUNTER_FLOATS) return CAPMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t NR = (size_t)N * R;
    const int TN = T * N;
    float *P = s->partial;
    const int64_t cap = s->partial_capacity;
    float *slabs = P + CAPMI_WS_COUNTER_FLOATS;
    // d(logits), time-major [T,N,V1]
    RC(dlogits_bwd((r->mode & CAPMI_SELECT_RAW) && !r->teacher, s->sparse, g_seq_logp, r->seq_logp, r->live, s->dlogits, N, L, T,
                   V1, stream));
    {
        SegSpec a{s->dlogits, V1, w->logit_w, R, V1};                 // d_hdrop = dlogits W_logit   [TN,R]
        RC(gemm(stream, 0, 1, TN, R, s->d_hdrop, R, &a, 1, P, cap, 0, nullptr));
    }
    // BPTT.  Per step: cell (dh = d_hdrop * mask + the previous iteration's dh slabs) -> a2c dX as slabs, finished and published by
    // the attention Jacobian (d_ctx, d_att_h, d_e) -> dh_prev = d_att_h W_h2att + d_sums W_h2h as slabs for the next cell.
    int dh_splits = 0;
    for (int t = T - 1; t >= 0; --t) {
        const bool last = (t == T - 1);
        float *d_sums = s->d_sums + (size_t)t * N * 5 * R;
        float *d_att_h = s->d_att_h + (size_t)t * N * A;
        float *dc_in = s->dc + (size_t)((t + 1) & 1) * NR, *dc_out = s->dc + (size_t)(t & 1) * NR;
        RC(capmi_att2in2_cell_bwd(s->d_hdrop + (size_t)t * NR, r->drop_out ? r->drop_out + (size_t)t * NR : nullptr,
                                  last ? nullptr : slabs, dh_splits, (int64_t)NR, last ? nullptr : dc_in,
                                  r->saved + (size_t)t * N * 5 * R, r->c + (size_t)t * NR, r->c + (size_t)(t + 1) * NR, d_sums,
                                  dc_out, N, R, stream));
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
    const bool dw_ws = cap >= CAPMI_WS_COUNTER_FLOATS + (int64_t)B * K * A;
    float *dw_part = dw_ws ? slabs : nullptr;
    RC(capmi_attention_bwd_batched_ws(s->d_ctx, R, r->att_h, r->alpha, s->d_e, r->p_att, w->alpha_w, g->d_att, g->d_p_att,
                                      dw_ws ? nullptr : g->alpha_w, g->alpha_b, T, B, n, N, K, A, R, dw_part, stream));
    if (dw_part) RC(capmi_colsum(dw_part, B * K, A, A, g->alpha_w, 0, stream));
    // token embeddings: d_x = d_sums W_i2h, scattered through ReLU / dropout
    {
        SegSpec a{s->d_sums, 5 * R, w->i2h_w, E, 5 * R};
        RC(gemm(stream, 0, 1, TN, E, s->d_x, E, &a, 1, P, cap, 0, nullptr));
        HIP_RC(hipMemsetAsync(g->embed, 0, (size_t)V1 * E * sizeof(float), st));
        RC(capmi_embed_bwd(r->it_all, s->d_x, r->x, r->drop_xt, g->embed, TN, E, 1, stream));
    }
    // the five time-batched weight gradients (K = T*N rows) with their bias column sums as ONE grouped launch; h_prev of step t is
    // state slot t, i.e. slots 0..T-1 of h
    capmi_group_gemm grp[5] = {
        {s->dlogits, r->h_drop, g->logit_w, V1, R, R, TN, V1, R, 0, 0, nullptr},
        {s->d_sums, r->x, g->i2h_w, 5 * R, E, E, TN, 5 * R, E, 0, 0, nullptr},
        {s->d_sums, r->h, g->h2h_w, 5 * R, R, R, TN, 5 * R, R, 0, 0, nullptr},
        {s->d_sums + 3 * R, r->ctx, g->a2c_w, 5 * R, R, R, TN, 2 * R, R, 0, 0, nullptr},
        {s->d_att_h, r->h, g->h2att_w, A, R, R, TN, A, R, 0, 0, nullptr}};
    struct { float *out; const float *in; int ld, cols; } bias[5] = {
        {g->logit_b, s->dlogits, V1, V1}, {g->i2h_b, s->d_sums, 5 * R, 5 * R}, {g->h2h_b, s->d_sums, 5 * R, 5 * R},
        {g->a2c_b, s->d_sums + 3 * R, 5 * R, 2 * R}, {g->h2att_b, s->d_att_h, A, A}};
    for (int i = 0; i < 5; ++i) {
        if (aligned16(bias[i].out)) grp[i].colsum = bias[i].out;
        else RC(capmi_colsum(bias[i].in, TN, bias[i].cols, bias[i].ld, bias[i].out, 0, stream));
    }
    // (the K-slice pieces go behind alpha_net's partial rows: the column sum above is enqueued before, but keep them apart anyway)
    const int64_t skip = CAPMI_WS_COUNTER_FLOATS + (((int64_t)B * K * A + 1023) & ~(int64_t)1023);
    RC(capmi_gemm_group_tn(grp, 5, cap > skip ? P + skip : nullptr, cap > skip ? cap - skip : 0, stream));
    return 0;
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
    SegSpec l{h_dst, R, w->logit_w, R, R};
    return gemm(stream, 0, 0, rows, V1, s->logits, V1, &l, 1, ws.p1, ws.cap1, 0, nullptr, w->logit_b);
}

}  // extern "C"
