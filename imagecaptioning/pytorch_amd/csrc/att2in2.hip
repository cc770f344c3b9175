// Att2in2 decoder on gfx950: cell kernels, whole-rollout drivers (forward and BPTT) and a single decode step.
// Replaces Att2in2Core.forward (AttModel.py:750-790) under Att2in2Model (AttModel.py:854-859) and the time loops of
// AttModel._forward / _sample for that model.  The recurrence is the NewFC maxout cell (newfc.hip) whose candidate half also
// receives a2c(att_res); the attention is UpDown's additive region attention (attention.hip), queried with the state BEFORE
// the step.  Same structure as the NewFC / UpDown drivers: one host call per rollout, no host sync, time-batched weight
// gradients as one grouped launch.
#include "capmi_common.h"
#include "../../../include/capmi.h"

using namespace capmi;

namespace {

#define RC(x)                 \
    do {                      \
        int rc__ = (x);       \
        if (rc__) return rc__;\
    } while (0)

inline int grid_for(size_t work) {
    size_t b = (work + 255) / 256;
    if (b > 2048) b = 2048;
    return (int)(b < 1 ? 1 : b);
}

// sums[r, q*R + j] = sum_s partial[s][r][q*R + j] (+ addend) + b_i2h + b_h2h, and for q = 3, 4 (the candidate half)
// + sum_s partial2[s][r][(q-3)*R + j] + b_a2c.  saved = (sig(in), sig(f), sig(out), cand_a, cand_b).
__global__ void att2in2_cell_fwd_kernel(const float *__restrict__ partial, int splits, const float *__restrict__ partial2,
                                        int splits2, const float *__restrict__ addend, const float *__restrict__ b_i2h,
                                        const float *__restrict__ b_h2h, const float *__restrict__ b_a2c,
                                        const float *__restrict__ c_prev, float *__restrict__ h, float *__restrict__ c,
                                        float *__restrict__ saved, const float *__restrict__ out_mask,
                                        float *__restrict__ h_drop, int N, int R) {
    const size_t total = (size_t)N * R, slab = (size_t)N * 5 * R, slab2 = (size_t)N * 2 * R;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / R), j = (int)(i % R);
        float s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const size_t col = (size_t)q * R + j;
            float v = 0.f;
            for (int k = 0; k < splits; ++k) v += partial[(size_t)k * slab + (size_t)r * 5 * R + col];
            if (addend) v += addend[(size_t)r * 5 * R + col];
            if (b_i2h) v += b_i2h[col];
            if (b_h2h) v += b_h2h[col];
            if (q >= 3) {
                const size_t col2 = (size_t)(q - 3) * R + j;
                float a = 0.f;
                for (int k = 0; k < splits2; ++k) a += partial2[(size_t)k * slab2 + (size_t)r * 2 * R + col2];
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

// dh = dh_a (* dh_a_mask) + sum_s dh_b[s][r][j] (the dX GEMM of the step after, left as K-slice slabs); d_sums [N,5R], dc_prev.
__global__ void att2in2_cell_bwd_kernel(const float *__restrict__ dh_a, const float *__restrict__ dh_a_mask,
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

struct SegSpec {
    const float *A; int lda; const float *B; int ldb; int K;
};
int gemm(void *stream, int al, int bl, int M, int N, float *C, int ldc, const SegSpec *segs, int nseg, float *partial,
         int64_t cap, int defer, int *splits_used, const float *bias = nullptr) {
    capmi_gemm_desc d{};
    d.nseg = nseg;
    for (int i = 0; i < nseg; ++i) {
        d.seg[i].A = segs[i].A; d.seg[i].lda = segs[i].lda; d.seg[i].B = segs[i].B; d.seg[i].ldb = segs[i].ldb;
        d.seg[i].K = segs[i].K; d.seg[i].a_row_div = 1;
    }
    d.a_layout = al; d.b_layout = bl; d.M = M; d.N = N; d.C = C; d.ldc = ldc; d.bias = bias;
    d.partial = partial; d.partial_capacity = cap; d.splits = 0; d.defer_reduce = defer;
    const int rc = capmi_gemm_f32(&d, stream);
    if (splits_used) *splits_used = d.splits_used;
    return rc;
}

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

int capmi_att2in2_cell_fwd(const float *partial, int splits, const float *partial2, int splits2, const float *addend,
                           const float *b_i2h, const float *b_h2h, const float *b_a2c, const float *c_prev, float *h, float *c,
                           float *saved, const float *out_mask, float *h_drop, int N, int R, void *stream) {
    if (!partial || splits < 1 || splits2 < 0 || (splits2 > 0 && !partial2) || !c_prev || !h || !c || !saved || N <= 0 || R <= 0)
        return CAPMI_EINVAL;
    hipLaunchKernelGGL(att2in2_cell_fwd_kernel, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, partial,
                       splits, partial2, splits2, addend, b_i2h, b_h2h, b_a2c, c_prev, h, c, saved, out_mask, h_drop, N, R);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_att2in2_cell_bwd(const float *dh_a, const float *dh_a_mask, const float *dh_b, int b_splits, int64_t b_stride,
                           const float *dc_next, const float *saved, const float *c_prev, const float *c_new, float *d_sums,
                           float *dc_prev, int N, int R, void *stream) {
    if (!saved || !c_prev || !c_new || !d_sums || !dc_prev || N <= 0 || R <= 0 || (dh_b && (b_splits < 1 || b_stride < (int64_t)N * R)))
        return CAPMI_EINVAL;
    hipLaunchKernelGGL(att2in2_cell_bwd_kernel, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, dh_a,
                       dh_a_mask, dh_b, b_splits, b_stride, dc_next, saved, c_prev, c_new, d_sums, dc_prev, N, R);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_att2in2_rollout_fwd(const capmi_att2in2_weights *w, capmi_att2in2_rollout *r, void *stream) {
    if (!w || !r) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, K = r->K, A = r->A, R = r->R, E = r->E, V1 = r->V1, T = r->T, L = r->L;
    if (B <= 0 || n <= 0 || N != B * n || K <= 0 || A <= 0 || T <= 0 || L < T || !r->partial || !r->att || !r->p_att)
        return CAPMI_EINVAL;
    if (((r->mode & 255) == 2 || r->teacher) && !r->forced) return CAPMI_EINVAL;
    if (r->ss_mode && !r->teacher) return CAPMI_EINVAL;
    Carve ws;
    if (!carve(r->partial, r->partial_capacity, &ws)) return CAPMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
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
    (void)st;
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
    if ((r->mode & CAPMI_SELECT_RAW) && !r->teacher) {
        capmi_sparse_logp_grad sp = s->sparse ? *s->sparse : capmi_sparse_logp_grad{};
        sp.raw = 1;
        RC(capmi_logsoftmax_bwd_sparse(&sp, g_seq_logp, r->seq_logp, r->live, s->dlogits, N, L, T, V1, stream));
    } else if (s->sparse) RC(capmi_logsoftmax_bwd_sparse(s->sparse, g_seq_logp, r->seq_logp, r->live, s->dlogits, N, L, T, V1, stream));
    else RC(capmi_logsoftmax_bwd(g_seq_logp, r->seq_logp, r->live, s->dlogits, N, L, T, V1, stream));
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
        hipError_t e = hipMemsetAsync(g->embed, 0, (size_t)V1 * E * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
        RC(capmi_embed_bwd(r->it_all, s->d_x, r->x, r->drop_xt, g->embed, TN, E, 1, stream));
    }
    // the five time-batched weight gradients (K = T*N rows) with their bias column sums as ONE grouped launch; h_prev of step t is
    // state slot t, i.e. slots 0..T-1 of h
    auto al16 = [](const float *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
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
        if (al16(bias[i].out)) grp[i].colsum = bias[i].out;
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
