// AdaAtt decoder on gfx950 ("Knowing when to look"): the visual-sentinel LSTM cell, whole-rollout drivers (forward and BPTT) and
// a single decode step.  Replaces AdaAttCore.forward (AttModel.py:604-613) = AdaAtt_lstm (:451-537, one layer) + AdaAtt_attention
// (:539-602) under AdaAttModel / AdaAttMOModel (:843-852) and the time loops of AttModel._forward / _sample for them.  The
// sentinel attention kernels live beside the additive attention they extend (attention.hip).  One host call per rollout, no
// host sync, time-batched weight gradients as one grouped launch; the driver plumbing around the step is rollout_common.h's.
//
// What the structure of this model gives the driver:
//  * v2h(fc) and r_v2h(fc) do not depend on the step: the caller hands them in as fc_gates [B, G+R] (with all six gate biases
//    folded in), added per image inside the cell;
//  * (w2h | r_w2h) and (h2h | r_h2h) are stacked by rows, so gates and sentinel gate come out of ONE GEMM per step, and under
//    teacher forcing the x half of all T steps is one GEMM (xin);
//  * the recurrence runs through (h, c) only: the attention output of a step feeds that step's logits and nothing else.  The
//    backward therefore runs logit -> att2h -> sentinel attention -> ho / fr projections for ALL T steps as time-batched launches
//    and only the cell (one launch + one dX GEMM per step) walks back through time.
#include "rollout_common.h"

using namespace capmi;

namespace {

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

// MO: maxout candidate (adaattmo, 5R gate columns) instead of tanh (adaatt, 4R); the sentinel gate is the last R-block.
// saved [N, W] = (sig(in), sig(f), sig(out), cand: tanh value | the two maxout inputs, sig(sentinel)),  W = G + R.
template <bool MO>
__global__ void adaatt_cell_fwd_kernel(const float *__restrict__ partial, int splits, const float *__restrict__ addend,
                                       const float *__restrict__ fc_gates, int n, const float *__restrict__ c_prev,
                                       float *__restrict__ h, float *__restrict__ c, float *__restrict__ saved,
                                       const float *__restrict__ drop_h, const float *__restrict__ drop_fake,
                                       float *__restrict__ h_drop, float *__restrict__ fake_drop, int N, int R) {
    constexpr int NQ = MO ? 6 : 5;
    const size_t W = (size_t)NQ * R, total = (size_t)N * R, slab = (size_t)N * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / R), j = (int)(i % R);
        float s[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const size_t col = (size_t)q * R + j;
            float v = slab_sum(partial, splits, slab, (size_t)r * W + col);
            if (addend) v += addend[(size_t)r * W + col];
            if (fc_gates) v += fc_gates[(size_t)(r / n) * W + col];
            s[q] = v;
        }
        const float ig = sigmoid_f(s[0]), fg = sigmoid_f(s[1]), og = sigmoid_f(s[2]);
        const float cand = MO ? fmaxf(s[3], s[4]) : tanh_f(s[3]);
        const float sg = sigmoid_f(s[NQ - 1]);
        const float cn = fg * c_prev[i] + ig * cand;
        const float tc = tanh_f(cn);
        const float hn = og * tc, fk = sg * tc;
        c[i] = cn;
        h[i] = hn;
        float *sv = saved + (size_t)r * W + j;
        sv[0] = ig; sv[R] = fg; sv[2 * (size_t)R] = og;
        if (MO) { sv[3 * (size_t)R] = s[3]; sv[4 * (size_t)R] = s[4]; }
        else sv[3 * (size_t)R] = cand;
        sv[(size_t)(NQ - 1) * R] = sg;
        h_drop[i] = drop_h ? hn * drop_h[i] : hn;
        fake_drop[i] = drop_fake ? fk * drop_fake[i] : fk;
    }
}

template <bool MO>
__global__ void adaatt_cell_bwd_kernel(const float *__restrict__ dh_a, const float *__restrict__ dh_a_mask,
                                       const float *__restrict__ d_fake, const float *__restrict__ d_fake_mask,
                                       const float *__restrict__ dh_b, int b_splits, int64_t b_stride,
                                       const float *__restrict__ dc_next, const float *__restrict__ saved,
                                       const float *__restrict__ c_prev, const float *__restrict__ c_new,
                                       float *__restrict__ d_sums, float *__restrict__ dc_prev, int N, int R) {
    constexpr int NQ = MO ? 6 : 5;
    const size_t W = (size_t)NQ * R, total = (size_t)N * R;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / R), j = (int)(i % R);
        float dh = 0.f, df = 0.f;
        if (dh_a) dh += dh_a_mask ? dh_a[i] * dh_a_mask[i] : dh_a[i];
        if (dh_b)
            for (int k = 0; k < b_splits; ++k) dh += dh_b[(size_t)k * b_stride + i];
        if (d_fake) df = d_fake_mask ? d_fake[i] * d_fake_mask[i] : d_fake[i];
        const float *sv = saved + (size_t)r * W + j;
        const float ig = sv[0], fg = sv[R], og = sv[2 * (size_t)R], sg = sv[(size_t)(NQ - 1) * R];
        const float ca = sv[3 * (size_t)R], cb = MO ? sv[4 * (size_t)R] : 0.f;
        const float cand = MO ? fmaxf(ca, cb) : ca;
        const float tc = tanh_f(c_new[i]);
        float dc = (dh * og + df * sg) * (1.f - tc * tc);
        if (dc_next) dc += dc_next[i];
        float *ds = d_sums + (size_t)r * W + j;
        ds[0] = dc * cand * ig * (1.f - ig);
        ds[R] = dc * c_prev[i] * fg * (1.f - fg);
        ds[2 * (size_t)R] = dh * tc * og * (1.f - og);
        const float dcand = dc * ig;
        if (MO) {       // torch.max(a, b) routes the gradient to the larger chunk
            ds[3 * (size_t)R] = ca >= cb ? dcand : 0.f;
            ds[4 * (size_t)R] = ca >= cb ? 0.f : dcand;
        } else {
            ds[3 * (size_t)R] = dcand * (1.f - cand * cand);
        }
        ds[(size_t)(NQ - 1) * R] = df * tc * sg * (1.f - sg);
        dc_prev[i] = dc * fg;
    }
}

// y_t = act(sum_s slabs[s] + bias), y = y_t * mask for up to two independent [N, C] products of equal shape (fr_linear |
// ho_linear; att2h alone): the epilogue of GEMMs left as K-slice slabs
struct ActSeg {
    const float *slabs; int splits; const float *bias, *mask; float *y_t, *y; int tanh_;
};
__global__ void adaatt_act_fwd_kernel(ActSeg s0, ActSeg s1, int nseg, int N, int C) {
    const size_t per = (size_t)N * C, total = per * nseg;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const bool second = i >= per;
        const ActSeg &s = second ? s1 : s0;
        const size_t e = second ? i - per : i;
        float v = slab_sum(s.slabs, s.splits, per, e);
        if (s.bias) v += s.bias[e % C];
        v = s.tanh_ ? tanh_f(v) : fmaxf(v, 0.f);
        if (s.y_t) s.y_t[e] = v;
        s.y[e] = s.mask ? v * s.mask[e] : v;
    }
}

// in place: d *= mask * act'(ref); tanh: ref = the value before the mask; relu: ref = the output (positive where it passed)
struct ActBwdSeg {
    float *d; const float *mask, *ref; int tanh_;
};
__global__ void adaatt_act_bwd_kernel(ActBwdSeg s0, ActBwdSeg s1, int nseg, size_t per) {
    const size_t total = per * nseg;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const bool second = i >= per;
        const ActBwdSeg &s = second ? s1 : s0;
        const size_t e = second ? i - per : i;
        float g = s.d[e];
        if (s.mask) g *= s.mask[e];
        const float y = s.ref[e];
        g = s.tanh_ ? g * (1.f - y * y) : (y > 0.f ? g : 0.f);
        s.d[e] = g;
    }
}

int act_fwd(const ActSeg &s0, const ActSeg *s1, int N, int C, void *stream) {
    const int nseg = s1 ? 2 : 1;
    hipLaunchKernelGGL(adaatt_act_fwd_kernel, dim3(grid_for((size_t)N * C * nseg)), dim3(256), 0, (hipStream_t)stream, s0,
                       s1 ? *s1 : s0, nseg, N, C);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int act_bwd(const ActBwdSeg &s0, const ActBwdSeg *s1, size_t per, void *stream) {
    const int nseg = s1 ? 2 : 1;
    hipLaunchKernelGGL(adaatt_act_bwd_kernel, dim3(grid_for(per * nseg)), dim3(256), 0, (hipStream_t)stream, s0, s1 ? *s1 : s0,
                       nseg, per);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

struct StepBufs {
    const float *x, *xin, *h_prev, *c_prev;
    float *h, *c, *saved, *h_drop, *fake_drop, *fr, *ho_t, *ho, *fr_e, *ho_e, *pi, *ctx, *out_t, *out_drop;
    const float *m_h, *m_fake, *m_fr, *m_ho, *m_out;
    const capmi_tile_drop *tile;
};

// One recurrent step without the vocabulary projection.  Launch chain: gate GEMM -> cell -> fr_linear, ho_linear GEMMs -> their
// activations (one launch) -> fr_embed, ho_embed GEMMs -> sentinel attention (finishes both) -> att2h GEMM -> its activation.
int core_step(const capmi_adaatt_weights *w, const Carve &ws, int B, int n, int N, int K, int A, int R, int E, int maxout,
              const float *fc_gates, const float *att, const float *p_att, const float *att_mask, const StepBufs &b,
              void *stream) {
    float *slabs1 = ws.p1 + CAPMI_WS_COUNTER_FLOATS, *slabs2 = ws.p2 + CAPMI_WS_COUNTER_FLOATS;
    const int W = (maxout ? 6 : 5) * R;
    int splits = 1, splits2 = 1;
    if (b.xin) {
        SegSpec s{b.h_prev, R, w->hw, R, R};
        RC(gemm(stream, 0, 0, N, W, ws.p1, W, &s, 1, ws.p1, ws.cap1, 1, &splits));
    } else {
        SegSpec s[2] = {{b.x, E, w->xw, E, E}, {b.h_prev, R, w->hw, R, R}};
        RC(gemm(stream, 0, 0, N, W, ws.p1, W, s, 2, ws.p1, ws.cap1, 1, &splits));
    }
    RC(capmi_adaatt_cell_fwd(slabs1, splits, b.xin, fc_gates, n, b.c_prev, b.h, b.c, b.saved, b.m_h, b.m_fake, b.h_drop,
                             b.fake_drop, N, R, maxout, stream));
    {
        SegSpec s1{b.fake_drop, R, w->fr_w, R, R}, s2{b.h_drop, R, w->ho_w, R, R};
        RC(gemm(stream, 0, 0, N, E, ws.p1, E, &s1, 1, ws.p1, ws.cap1, 1, &splits));
        RC(gemm(stream, 0, 0, N, E, ws.p2, E, &s2, 1, ws.p2, ws.cap2, 1, &splits2));
        const ActSeg a1{slabs1, splits, w->fr_b, b.m_fr, nullptr, b.fr, 0}, a2{slabs2, splits2, w->ho_b, b.m_ho, b.ho_t, b.ho, 1};
        RC(act_fwd(a1, &a2, N, E, stream));
    }
    {
        SegSpec s1{b.fr, E, w->fre_w, E, E}, s2{b.ho, E, w->hoe_w, E, E};
        RC(gemm(stream, 0, 0, N, A, ws.p1, A, &s1, 1, ws.p1, ws.cap1, 1, &splits));
        RC(gemm(stream, 0, 0, N, A, ws.p2, A, &s2, 1, ws.p2, ws.cap2, 1, &splits2));
        RC(capmi_sentinel_attention_fwd(slabs1, splits, (int64_t)N * A, w->fre_b, slabs2, splits2, (int64_t)N * A, w->hoe_b,
                                        b.fr_e, b.ho_e, b.fr, b.ho, p_att, att, att_mask, w->alpha_w, w->alpha_b, b.tile, b.pi,
                                        b.ctx, B, n, K, A, R, stream));
    }
    SegSpec s{b.ctx, R, w->att2h_w, R, R};
    RC(gemm(stream, 0, 0, N, R, ws.p1, R, &s, 1, ws.p1, ws.cap1, 1, &splits));
    const ActSeg a{slabs1, splits, w->att2h_b, b.m_out, b.out_t, b.out_drop, 1};
    return act_fwd(a, nullptr, N, R, stream);
}

}  // namespace

extern "C" {

int capmi_adaatt_cell_fwd(const float *partial, int splits, const float *addend, const float *fc_gates, int n,
                          const float *c_prev, float *h, float *c, float *saved, const float *drop_h, const float *drop_fake,
                          float *h_drop, float *fake_drop, int N, int R, int maxout, void *stream) {
    if (!partial || splits < 1 || !c_prev || !h || !c || !saved || !h_drop || !fake_drop || N <= 0 || R <= 0 ||
        (fc_gates && (n <= 0 || N % n)))
        return CAPMI_EINVAL;
    if (maxout)
        hipLaunchKernelGGL(adaatt_cell_fwd_kernel<true>, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, partial,
                           splits, addend, fc_gates, n, c_prev, h, c, saved, drop_h, drop_fake, h_drop, fake_drop, N, R);
    else
        hipLaunchKernelGGL(adaatt_cell_fwd_kernel<false>, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, partial,
                           splits, addend, fc_gates, n, c_prev, h, c, saved, drop_h, drop_fake, h_drop, fake_drop, N, R);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_adaatt_cell_bwd(const float *dh_a, const float *dh_a_mask, const float *d_fake, const float *d_fake_mask,
                          const float *dh_b, int b_splits, int64_t b_stride, const float *dc_next, const float *saved,
                          const float *c_prev, const float *c_new, float *d_sums, float *dc_prev, int N, int R, int maxout,
                          void *stream) {
    if (!saved || !c_prev || !c_new || !d_sums || !dc_prev || N <= 0 || R <= 0 ||
        (dh_b && (b_splits < 1 || b_stride < (int64_t)N * R)))
        return CAPMI_EINVAL;
    if (maxout)
        hipLaunchKernelGGL(adaatt_cell_bwd_kernel<true>, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, dh_a,
                           dh_a_mask, d_fake, d_fake_mask, dh_b, b_splits, b_stride, dc_next, saved, c_prev, c_new, d_sums, dc_prev,
                           N, R);
    else
        hipLaunchKernelGGL(adaatt_cell_bwd_kernel<false>, dim3(grid_for((size_t)N * R)), dim3(256), 0, (hipStream_t)stream, dh_a,
                           dh_a_mask, d_fake, d_fake_mask, dh_b, b_splits, b_stride, dc_next, saved, c_prev, c_new, d_sums, dc_prev,
                           N, R);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_adaatt_rollout_fwd(const capmi_adaatt_weights *w, capmi_adaatt_rollout *r, void *stream) {
    if (!w || !r) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, K = r->K, A = r->A, R = r->R, E = r->E, V1 = r->V1, T = r->T;
    if (B <= 0 || n <= 0 || N != B * n || K <= 0 || A <= 0 || !r->partial || !r->att || !r->p_att || !r->fc_gates || E != R || A != R)
        return CAPMI_EINVAL;
    const SelectIO io = select_io(r);
    RC(check_rollout_io(io));
    if (!r->drop_tile && (r->tile_p < 0.f || r->tile_p >= 1.f)) return CAPMI_EINVAL;
    Carve ws;
    if (!carve(r->partial, r->partial_capacity, &ws)) return CAPMI_EINVAL;
    const int W = (r->maxout ? 6 : 5) * R;
    const size_t NR = (size_t)N * R, NE = (size_t)N * E, NA = (size_t)N * A, NW = (size_t)N * W, NK1 = (size_t)N * (K + 1);
    // teacher forcing knows every input token up front: the (w2h | r_w2h) half of all T steps is ONE GEMM over T*N rows
    const bool batched_x = r->teacher && !scheduled(io) && r->xin;
    const EmbedSpec emb{w->embed, E, 1, r->drop_xt, r->x, true};
    RC(capmi_rollout_init(r->h, r->c, nullptr, nullptr, (int64_t)NR, r->it, r->unfinished, N, stream));    // state 0, BOS
    RC(teacher_inputs(io, emb, w->xw, W, batched_x ? r->xin : nullptr, ws.p1, ws.cap1, stream));
    for (int t = 0; t < T; ++t) {
        capmi_tile_drop tile{};
        tile.mask = r->drop_tile ? r->drop_tile + t * NK1 * A : nullptr;
        tile.p = r->drop_tile ? 0.f : r->tile_p;
        tile.seed = r->tile_seed;
        tile.row0 = (int64_t)t * N;
        StepBufs b{};
        b.x = r->x + t * NE; b.xin = batched_x ? r->xin + t * NW : nullptr;
        b.h_prev = r->h + t * NR; b.c_prev = r->c + t * NR; b.h = r->h + (t + 1) * NR; b.c = r->c + (t + 1) * NR;
        b.saved = r->saved + t * NW; b.h_drop = r->h_drop + t * NR; b.fake_drop = r->fake_drop + t * NR;
        b.fr = r->fr + t * NE; b.ho_t = r->ho_t + t * NE; b.ho = r->ho + t * NE; b.fr_e = r->fr_e + t * NA; b.ho_e = r->ho_e + t * NA;
        b.pi = r->pi + t * NK1; b.ctx = r->ctx + t * NR; b.out_t = r->out_t + t * NR; b.out_drop = r->out_drop + t * NR;
        b.m_h = r->drop_h ? r->drop_h + t * NR : nullptr; b.m_fake = r->drop_fake ? r->drop_fake + t * NR : nullptr;
        b.m_fr = r->drop_fr ? r->drop_fr + t * NE : nullptr; b.m_ho = r->drop_ho ? r->drop_ho + t * NE : nullptr;
        b.m_out = r->drop_out ? r->drop_out + t * NR : nullptr;
        b.tile = (tile.mask || tile.p > 0.f) ? &tile : nullptr;
        RC(core_step(w, ws, B, n, N, K, A, R, E, r->maxout, r->fc_gates, r->att, r->p_att, r->att_mask, b, stream));
        int splits = 1;
        RC(logit_slabs(stream, b.out_drop, w->logit_w, N, V1, R, ws.p1, ws.cap1, &splits));
        RC(select_step(io, t, ws.p1 + CAPMI_WS_COUNTER_FLOATS, splits, w->logit_b, emb, stream));
    }
    return 0;
}

int capmi_adaatt_rollout_bwd(const capmi_adaatt_weights *w, const capmi_adaatt_rollout *r, const float *g_seq_logp,
                             capmi_adaatt_bwd_scratch *s, capmi_adaatt_grads *g, void *stream) {
    if (!w || !r || (!g_seq_logp && !(s && s->sparse)) || !s || !g) return CAPMI_EINVAL;
    const int B = r->B, n = r->n, N = r->N, K = r->K, A = r->A, R = r->R, E = r->E, V1 = r->V1, T = r->T;
    if (!s->partial || s->partial_capacity <= CAPMI_WS_COUNTER_FLOATS || E != R || A != R) return CAPMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int G = (r->maxout ? 5 : 4) * R, W = G + R;
    const size_t NR = (size_t)N * R, NW = (size_t)N * W;
    const int TN = T * N;
    float *P = s->partial;
    const int64_t cap = s->partial_capacity;
    float *slabs = P + CAPMI_WS_COUNTER_FLOATS;
    capmi_tile_drop tile{};
    tile.mask = r->drop_tile;
    tile.p = r->drop_tile ? 0.f : r->tile_p;
    tile.seed = r->tile_seed;
    const capmi_tile_drop *td = (tile.mask || tile.p > 0.f) ? &tile : nullptr;
    // ---- everything behind the cell, for all T steps at once ----------------------------------------------------------------
    RC(logit_bwd_head(select_io(r), s->sparse, g_seq_logp, s->dlogits, w->logit_w, R, s->d_out, P, cap, stream));   // d_out_drop
    {
        const ActBwdSeg ab{s->d_out, r->drop_out, r->out_t, 1};         // through the output dropout and att2h's tanh, in place
        RC(act_bwd(ab, nullptr, (size_t)TN * R, stream));
        SegSpec c{s->d_out, R, w->att2h_w, R, R};                      // d_ctx = d_out W_att2h
        RC(gemm(stream, 0, 1, TN, R, s->d_ctx, R, &c, 1, P, cap, 0, nullptr));
    }
    RC(capmi_sentinel_attention_bwd(s->d_ctx, r->fr, r->fr_e, r->ho_e, r->pi, r->p_att, r->att, w->alpha_w, td, s->d_e, s->d_hoe,
                                    s->d_fre, s->d_fr, T, B, n, K, A, R, stream));
    {
        // d_fr += d_fre W_fr_embed;  d_ho = d_ctx (the residual) + d_hoe W_ho_embed;  then through ReLU / tanh and their masks
        SegSpec a{s->d_fre, A, w->fre_w, E, A}, c{s->d_hoe, A, w->hoe_w, E, A};
        RC(gemm(stream, 0, 1, TN, E, s->d_fr, E, &a, 1, P, cap, 0, nullptr, nullptr, nullptr, 1));
        HIP_RC(hipMemcpyAsync(s->d_ho, s->d_ctx, (size_t)TN * R * sizeof(float), hipMemcpyDeviceToDevice, st));
        RC(gemm(stream, 0, 1, TN, E, s->d_ho, E, &c, 1, P, cap, 0, nullptr, nullptr, nullptr, 1));
        const ActBwdSeg b1{s->d_fr, r->drop_fr, r->fr, 0}, b2{s->d_ho, r->drop_ho, r->ho_t, 1};
        RC(act_bwd(b1, &b2, (size_t)TN * E, stream));
        SegSpec f{s->d_fr, E, w->fr_w, R, E}, h{s->d_ho, E, w->ho_w, R, E};
        RC(gemm(stream, 0, 1, TN, R, s->d_fakedrop, R, &f, 1, P, cap, 0, nullptr));
        RC(gemm(stream, 0, 1, TN, R, s->d_hdrop, R, &h, 1, P, cap, 0, nullptr));
    }
    // ---- BPTT through the cell: dh = d_hdrop * mask + the previous iteration's dh slabs; dh_prev = d_sums (h2h | r_h2h) ----------
    int dh_splits = 0;
    for (int t = T - 1; t >= 0; --t) {
        const bool last = (t == T - 1);
        float *d_sums = s->d_sums + t * NW;
        RC(capmi_adaatt_cell_bwd(s->d_hdrop + t * NR, r->drop_h ? r->drop_h + t * NR : nullptr, s->d_fakedrop + t * NR,
                                 r->drop_fake ? r->drop_fake + t * NR : nullptr, last ? nullptr : slabs, dh_splits, (int64_t)NR,
                                 pp_in(s->dc, t, T, NR), r->saved + t * NW, r->c + t * NR, r->c + (t + 1) * NR, d_sums,
                                 pp_out(s->dc, t, NR), N, R, r->maxout, stream));
        if (t > 0) {       // the state before step 0 is the constant zero
            SegSpec a{d_sums, W, w->hw, R, W};
            RC(gemm(stream, 0, 1, N, R, P, R, &a, 1, P, cap, 1, &dh_splits));
        }
    }
    // ---- time-batched parameter / feature gradients ------------------------------------------------------------------------------
    const int64_t dw_floats = (int64_t)B * (K + 1) * A;
    float *dw_part = alpha_dw_part(P, cap, dw_floats);
    RC(capmi_sentinel_attention_bwd_batched(s->d_ctx, r->fr_e, r->ho_e, r->pi, s->d_e, r->p_att, w->alpha_w, td, g->d_att,
                                            g->d_p_att, dw_part ? nullptr : g->alpha_w, g->alpha_b, T, B, n, K, A, R, dw_part, stream));
    if (dw_part) RC(capmi_colsum(dw_part, B * (K + 1), A, A, g->alpha_w, 0, stream));
    // token embeddings: d_x = d_sums (w2h | r_w2h)
    RC(embed_grad(stream, SegSpec{s->d_sums, W, w->xw, E, W}, TN, E, s->d_x, r->it_all, r->x, r->drop_xt, 1, g->embed, V1, P, cap));
    RC(capmi_colsum(s->d_sums, TN, W, W, g->gate_b, 0, stream));
    RC(capmi_group_rowsum(s->d_sums, T, (int64_t)NW, B, n, W, g->d_fc_gates, stream));
    // the ten time-batched weight gradients (K = T*N rows) with their bias column sums as ONE grouped launch; h_prev of step t is
    // state slot t, i.e. slots 0..T-1 of h
    capmi_group_gemm grp[10] = {
        {s->dlogits, r->out_drop, g->logit_w, V1, R, R, TN, V1, R, 0, 0, nullptr},
        {s->d_out, r->ctx, g->att2h_w, R, R, R, TN, R, R, 0, 0, nullptr},
        {s->d_fre, r->fr, g->fre_w, A, E, E, TN, A, E, 0, 0, nullptr},
        {s->d_hoe, r->ho, g->hoe_w, A, E, E, TN, A, E, 0, 0, nullptr},
        {s->d_fr, r->fake_drop, g->fr_w, E, R, R, TN, E, R, 0, 0, nullptr},
        {s->d_ho, r->h_drop, g->ho_w, E, R, R, TN, E, R, 0, 0, nullptr},
        {s->d_sums, r->x, g->w2h_w, W, E, E, TN, G, E, 0, 0, nullptr},
        {s->d_sums + G, r->x, g->r_w2h_w, W, E, E, TN, R, E, 0, 0, nullptr},
        {s->d_sums, r->h, g->h2h_w, W, R, R, TN, G, R, 0, 0, nullptr},
        {s->d_sums + G, r->h, g->r_h2h_w, W, R, R, TN, R, R, 0, 0, nullptr}};
    const BiasCol bias[6] = {
        {g->logit_b, s->dlogits, V1, V1}, {g->att2h_b, s->d_out, R, R}, {g->fre_b, s->d_fre, A, A}, {g->hoe_b, s->d_hoe, A, A},
        {g->fr_b, s->d_fr, E, E}, {g->ho_b, s->d_ho, E, E}};
    return grouped_dw_with_bias(grp, 10, bias, 6, dw_floats, P, cap, stream);
}

int capmi_adaatt_decode_step(const capmi_adaatt_weights *w, capmi_adaatt_step *s, int rows, int rows_per_image,
                             const float *h_src, const float *c_src, float *h_dst, float *c_dst, void *stream) {
    if (!w || !s || rows <= 0 || rows_per_image <= 0 || rows != s->B * rows_per_image || !h_src || !c_src || !h_dst || !c_dst ||
        !s->partial || !s->it || !s->fc_gates || s->E != s->R || s->A != s->R)
        return CAPMI_EINVAL;
    const int B = s->B, K = s->K, A = s->A, R = s->R, E = s->E, V1 = s->V1;
    Carve ws;
    if (!carve(s->partial, s->partial_capacity, &ws)) return CAPMI_EINVAL;
    RC(capmi_embed_fwd(s->it, 1, nullptr, w->embed, nullptr, s->xt, rows, E, 1, stream));          // eval: ReLU, no dropout
    StepBufs b{};
    b.x = s->xt; b.h_prev = h_src; b.c_prev = c_src; b.h = h_dst; b.c = c_dst;
    b.saved = s->saved; b.h_drop = s->h_drop; b.fake_drop = s->fake_drop; b.fr = s->fr; b.ho_t = s->ho_t; b.ho = s->ho;
    b.fr_e = s->fr_e; b.ho_e = s->ho_e; b.pi = s->pi; b.ctx = s->ctx; b.out_t = s->out_t; b.out_drop = s->out_drop;
    RC(core_step(w, ws, B, rows_per_image, rows, K, A, R, E, s->maxout, s->fc_gates, s->att, s->p_att, s->att_mask, b, stream));
    return decode_logits(stream, s->out_drop, w->logit_w, w->logit_b, rows, V1, R, s->logits, ws.p1, ws.cap1);
}

}  // extern "C"
