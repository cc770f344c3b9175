// Driver plumbing shared by the LSTM rollout drivers (rollout.hip, newfc.hip, att2in2.hip, adaatt.hip): the tail of a forward
// step (logit slabs -> select, with the next step's embedding folded in), the teacher-forced prologue and the two ends of BPTT.
// Plain functions over plain structs; a family's file keeps what is its own.  Internal like host_common.h: not
// part of the C ABI in include/capmi.h.
#pragma once
#include "host_common.h"

// The split-K workspace in two regions, so that two independent GEMMs can both stay as K-slice slabs for the kernel that reads
// them together (Att2in2: gates | a2c; AdaAtt: fr | ho).
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

// The select side of a capmi_*_rollout: the fields all four structs share under the same names, and UpDown's extras (absent = 0).
struct SelectIO {
    int N, V1, T, L, mode;
    float temperature; const float *gumbel; uint64_t seed;
    const int64_t *forced; int forced_ld, teacher;
    const uint8_t *ss_mode;
    int64_t *seq; float *seq_logp, *sel_logp; uint8_t *live;
    int64_t *it; uint8_t *unfinished; int64_t *it_all;
    const uint8_t *row_mode;        // per-row mode of free-running steps
    capmi_sample_filter filter;     // top-k / top-p
    int raw_flag;                   // CAPMI_SELECT_RAW where the struct carries raw beside `mode`
    void *x_planes;                 // the folded embedding also as A planes
    int32_t *alive;                 // [L] early-exit words, one per step
};
template <typename Rollout>
inline SelectIO select_io(const Rollout *r) {
    SelectIO io{};
    io.N = r->N; io.V1 = r->V1; io.T = r->T; io.L = r->L; io.mode = r->mode; io.temperature = r->temperature;
    io.gumbel = r->gumbel; io.seed = r->seed; io.forced = r->forced; io.forced_ld = r->forced_ld; io.teacher = r->teacher;
    io.ss_mode = r->ss_mode; io.seq = r->seq; io.seq_logp = r->seq_logp; io.sel_logp = r->sel_logp; io.live = r->live;
    io.it = r->it; io.unfinished = r->unfinished; io.it_all = r->it_all;
    return io;
}
inline bool scheduled(const SelectIO &io) { return io.teacher && io.ss_mode; }
inline bool raw_rollout(const SelectIO &io) { return ((io.mode | io.raw_flag) & CAPMI_SELECT_RAW) && !io.teacher; }

// What every forward checks.  `mode` may carry CAPMI_SELECT_RAW, hence the & 255; UpDown's never does (raw arrives through
// raw_logits), so the mask changes nothing for it.
inline int check_rollout_io(const SelectIO &io) {
    if (io.N <= 0 || io.T <= 0 || io.L < io.T) return CAPMI_EINVAL;
    if (((io.mode & 255) == 2 || io.teacher) && !io.forced) return CAPMI_EINVAL;
    if (io.ss_mode && !io.teacher) return CAPMI_EINVAL;
    return 0;
}

// How a family embeds its input tokens: x [T,N,Edim] = relu?(table[token]) * mask.  fold_free: free-running steps get their
// input from the select launch of the step before, like scheduled-sampling steps always do.
struct EmbedSpec {
    const float *table; int Edim, relu;
    const float *mask;      // [T,N,Edim] or null
    float *x; bool fold_free;
};

// The select tail of step t: embed the chosen token as step t+1's input where that step takes it from here; the early-exit word.
inline capmi_next_embed next_embed(const SelectIO &io, int t, const EmbedSpec &e) {
    capmi_next_embed ne{};
    if (t + 1 < io.T && (io.teacher ? scheduled(io) : e.fold_free)) {
        const size_t o = (size_t)(t + 1) * io.N;
        ne.E = e.table; ne.Edim = e.Edim; ne.relu = e.relu;
        ne.mask = e.mask ? e.mask + o * e.Edim : nullptr;
        ne.x = e.x + o * e.Edim;
        ne.it_save = io.it_all ? io.it_all + o : nullptr;
        ne.x_planes = io.x_planes;
    }
    if (io.alive) ne.alive = io.alive + t;
    return ne;
}

// Log-softmax + choice + bookkeeping of step t from the logit GEMM's K-slice slabs.
inline int select_step(const SelectIO &io, int t, const float *slabs, int splits, const float *logit_b, const EmbedSpec &e,
                       void *stream) {
    const int N = io.N, V1 = io.V1;
    const float *gum = io.gumbel ? io.gumbel + (size_t)t * N * V1 : nullptr;
    const capmi_next_embed ne = next_embed(io, t, e);
    const capmi_next_embed *next = (ne.x || ne.alive) ? &ne : nullptr;     // (an empty tail and none are the same launch)
    if (scheduled(io) && t + 1 < io.T)
        // AttModel.py:145-154: the token chosen here is the INPUT of step t+1 -- forced[:, t+1] (ss_mode 2 rows) or a categorical
        // draw from this step's log-probs (ss_mode 1 rows, temperature 1); the same launch embeds it.  A drawn 0 does not end the
        // row: the labels decide that (no_finish_mask).
        return capmi_logsoftmax_select_partial(slabs, splits, (int64_t)N * V1, logit_b, N, V1, t, io.L, 2,
                                               io.ss_mode + (size_t)(t + 1) * N, 1.f, gum, io.seed, io.forced + 1, io.forced_ld, 1,
                                               io.seq, io.L, io.it, io.unfinished, io.seq_logp, io.sel_logp, io.live, next, nullptr,
                                               stream);
    const bool flt = io.filter.top_k > 0 || io.filter.top_p > 0.f;
    return capmi_logsoftmax_select_partial(slabs, splits, (int64_t)N * V1, logit_b, N, V1, t, io.L,
                                           io.teacher ? 2 : (io.mode | io.raw_flag), io.teacher ? nullptr : io.row_mode,
                                           io.temperature, gum, io.seed, io.forced, io.forced_ld, io.teacher ? 1 : 0, io.seq, io.L,
                                           io.it, io.unfinished, io.seq_logp, io.sel_logp, io.live, next, flt ? &io.filter : nullptr,
                                           stream);
}

// logits = h W_logit^T of one step, left as K-slice slabs behind the counters of `partial` for the select to assemble.
inline int logit_slabs(void *stream, const float *h, const float *logit_w, int N, int V1, int R, float *partial, int64_t cap,
                       int *splits, const void *h_planes = nullptr, const void *zero_planes = nullptr) {
    SegSpec s{h, R, logit_w, R, R, 1, h_planes};
    return gemm(stream, 0, 0, N, V1, partial, V1, &s, 1, partial, cap, 1, splits, nullptr, nullptr, 0, zero_planes);
}

// The same product finished, with its bias: the tail of a decode step.
inline int decode_logits(void *stream, const float *h, const float *logit_w, const float *logit_b, int rows, int V1, int R,
                         float *logits, float *partial, int64_t cap) {
    SegSpec s{h, R, logit_w, R, R};
    return gemm(stream, 0, 0, rows, V1, logits, V1, &s, 1, partial, cap, 0, nullptr, logit_b);
}

// The inputs of a rollout that embeds with ReLU.  Teacher forcing knows every token up front: all T steps are embedded here, and
// with `xin` the input half of the gates of all of them is ONE GEMM over T*N rows, xin [T*N, W] = x xw^T.  Otherwise step 0 only:
// BOS (free-running) or forced[:, 0] (scheduled sampling); later inputs come from the select's tail.
inline int teacher_inputs(const SelectIO &io, const EmbedSpec &e, const float *xw, int W, float *xin, float *partial, int64_t cap,
                          void *stream) {
    const int N = io.N, E = e.Edim;
    if (!io.teacher || scheduled(io))
        return capmi_embed_fwd(io.teacher ? io.forced : io.it, io.teacher ? io.forced_ld : 1, io.it_all, e.table, e.mask, e.x, N, E,
                               e.relu, stream);
    for (int t = 0; t < io.T; ++t)
        RC(capmi_embed_fwd(io.forced + t, io.forced_ld, io.it_all + (size_t)t * N, e.table,
                           e.mask ? e.mask + (size_t)t * N * E : nullptr, e.x + (size_t)t * N * E, N, E, e.relu, stream));
    if (!xin) return 0;
    SegSpec s{e.x, E, xw, E, E};
    return gemm(stream, 0, 0, io.T * N, W, xin, W, &s, 1, partial, cap, 0, nullptr);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// The head of every BPTT: d(logits), time-major [T,N,V1], and d_hdrop [T*N,R] = dlogits W_logit.
inline int logit_bwd_head(const SelectIO &io, const capmi_sparse_logp_grad *sparse, const float *g_seq_logp, float *dlogits,
                          const float *logit_w, int R, float *d_hdrop, float *P, int64_t cap, void *stream) {
    RC(dlogits_bwd(raw_rollout(io), sparse, g_seq_logp, io.seq_logp, io.live, dlogits, io.N, io.L, io.T, io.V1, stream));
    SegSpec a{dlogits, io.V1, logit_w, R, io.V1, 1};
    return gemm(stream, 0, 1, io.T * io.N, R, d_hdrop, R, &a, 1, P, cap, 0, nullptr);
}

// Two [N,R] slots that BPTT ping-pongs a carried gradient through: step t reads what step t+1 wrote (nothing at the last step).
inline float *pp_out(float *buf, int t, size_t NR) { return buf + (size_t)(t & 1) * NR; }
inline const float *pp_in(const float *buf, int t, int T, size_t NR) {
    return t == T - 1 ? nullptr : buf + (size_t)((t + 1) & 1) * NR;
}

// Token-embedding gradient: d_x [TN,Edim] = the dX GEMM `dx`, then scattered into g_embed [V1,Edim] through ReLU / dropout.
inline int embed_grad(void *stream, const SegSpec &dx, int TN, int Edim, float *d_x, const int64_t *it_all, const float *x,
                      const float *mask, int relu, float *g_embed, int V1, float *P, int64_t cap) {
    RC(gemm(stream, 0, 1, TN, Edim, d_x, Edim, &dx, 1, P, cap, 0, nullptr));
    HIP_RC(hipMemsetAsync(g_embed, 0, (size_t)V1 * Edim * sizeof(float), (hipStream_t)stream));
    return capmi_embed_bwd(it_all, d_x, x, mask, g_embed, TN, Edim, relu, stream);
}

// alpha_net's weight gradient as one partial row per (image, region) at the head of the workspace, where it fits; then a
// capmi_colsum over those `floats`.
inline float *alpha_dw_part(float *P, int64_t cap, int64_t floats) {
    return cap >= CAPMI_WS_COUNTER_FLOATS + floats ? P + CAPMI_WS_COUNTER_FLOATS : nullptr;
}

// The time-batched weight gradients with their bias column sums as ONE grouped launch.  bias[i] goes with grp[i], i < n_bias,
// and rides in its staging waves where the target is 16-byte aligned (a launch of its own otherwise).  The K-slice pieces go
// behind the dw_floats of alpha_net's partial rows: their column sum is enqueued before, but keep them apart anyway.
struct BiasCol { float *out; const float *in; int ld, cols; };
inline int grouped_dw_with_bias(capmi_group_gemm *grp, int n, const BiasCol *bias, int n_bias, int64_t dw_floats, float *P,
                                int64_t cap, void *stream) {
    for (int i = 0; i < n_bias; ++i) {
        if (aligned16(bias[i].out)) grp[i].colsum = bias[i].out;
        else RC(capmi_colsum(bias[i].in, grp[i].K, bias[i].cols, bias[i].ld, bias[i].out, 0, stream));
    }
    const int64_t skip = CAPMI_WS_COUNTER_FLOATS + ((dw_floats + 1023) & ~(int64_t)1023);
    return capmi_gemm_group_tn(grp, n, cap > skip ? P + skip : nullptr, cap > skip ? cap - skip : 0, stream);
}
