// Decode-time logits processors (gfx950): no_repeat_ngram_size, repetition_penalty, min_length and bad_words, applied in place to
// the [rows, V1] log-probability rows of one decode step.  Unlike decode_constrain_kernel (decode_opts.hip) this kernel sees a row's
// whole history in either form a decoder keeps it:
//   dense          seq [rows, seq_ld] int64, columns 0 .. t-1                       (decode.sample_steps)
//   back-pointer   the search core's per-step tables token int64 / parent int32 [L][B][W] (beam.py _search_loop): row b * W + j of
//                  step t > 0 is slot j of step t - 1, and the walk follows parent[s][b][slot] back to step 0
// One wave per row.  The history goes to LDS (at most 64 words); then, in this order: the penalty (one fp32 multiply per DISTINCT
// word), a barrier, and the three -inf rules -- so that a word that is both penalised and blocked ends at -inf.  A row whose
// history holds the end token 0 is left as it is.  Every store is bounds checked against V1: a table entry that is no token of
// the vocabulary is never used as a column.
#include "capmi_common.h"
#include "../../../include/capmi.h"

using namespace capmi;

namespace {

struct History {
    const int64_t *seq;          // dense, or null
    int seq_ld;
    const int64_t *token;        // back-pointer tables, when seq is null
    const int32_t *parent;
    int W;
};

__global__ __launch_bounds__(64) void logits_process_kernel(float *__restrict__ logp, int ld, int V1, int t, int L, int cur,
                                                            capmi_logits_proc p, History h, const int32_t *__restrict__ exempt,
                                                            int n_exempt) {
    __shared__ int hist[CAPMI_LP_HIST_MAX];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int img = r / cur;
    if (h.seq) {
        if (lane < t) {
            const int64_t v = h.seq[(size_t)r * h.seq_ld + lane];
            hist[lane] = (v >= 0 && v < V1) ? (int)v : -1;
        }
    } else if (lane == 0 && t > 0) {
        const int B = gridDim.x / cur;                       // t > 0: cur == W, r = img * W + slot of step t - 1
        int slot = r - img * cur;
        for (int s = t - 1; s >= 0; --s) {
            const size_t o = ((size_t)s * B + img) * h.W + slot;
            const int64_t v = h.token[o];
            hist[s] = (v >= 0 && v < V1) ? (int)v : -1;
            int par = h.parent[o];
            slot = par < 0 ? 0 : (par >= h.W ? h.W - 1 : par);
        }
    }
    __syncthreads();
    const int mine = lane < t ? hist[lane] : -1;
    if (__syncthreads_or(lane < t && mine == 0)) return;     // a finished row
    float *x = logp + (size_t)r * ld;

    if (p.repetition_penalty > 1.0f && mine > 0) {           // the first occurrence of a word penalises it, once
        bool first = true;
        for (int j = 0; j < lane; ++j) first &= hist[j] != mine;
        if (first) x[mine] = x[mine] * p.repetition_penalty;
    }
    __syncthreads();                                         // the penalty's stores are done before a rule below hits the same word

    if (lane == 0) {
        const int m = p.min_length < L - 1 ? p.min_length : L - 1;
        if (t < m) x[0] = -INFINITY;
    }
    const int n = p.no_repeat_ngram_size;
    if (n >= 1 && t >= n - 1) {
        const int *last = hist + (t - (n - 1));              // the n - 1 words the next one would follow
        for (int i = lane; i + n <= t; i += 64) {
            bool same = true;
            for (int k = 0; k < n - 1; ++k) same &= hist[i + k] == last[k];
            const int v = hist[i + n - 1];
            if (!same || v <= 0) continue;
            bool keep = false;                               // cbs: a word of the image's constraint lists is never blocked
            for (int e = 0; e < n_exempt; ++e) keep |= exempt[(size_t)img * n_exempt + e] == v;
            if (!keep) x[v] = -INFINITY;
        }
    }
    if (lane < p.n_bad) {
        const int len = p.bad_len[lane];
        if (len >= 1 && len <= CAPMI_LP_BAD_LEN && t >= len - 1) {
            const int *w = p.bad_words + lane * CAPMI_LP_BAD_LEN;
            bool same = true;
            for (int k = 0; k < len - 1; ++k) same &= hist[t - (len - 1) + k] == w[k];
            const int v = w[len - 1];
            if (same && v > 0 && v < V1) x[v] = -INFINITY;
        }
    }
}

}  // namespace

extern "C" {

int capmi_logits_process(float *logp, int ld, int rows, int V1, int t, int L, const capmi_logits_proc *p, const int64_t *seq,
                         int seq_ld, const int64_t *token, const int32_t *parent, int W, int cur, const int32_t *exempt,
                         int n_exempt, void *stream) {
    if (!logp || !p || rows <= 0 || V1 <= 0 || ld < V1 || L <= 0 || L > CAPMI_LP_HIST_MAX || t < 0 || t >= L) return CAPMI_EINVAL;
    if (cur <= 0 || rows % cur) return CAPMI_EINVAL;
    if (p->no_repeat_ngram_size < 0 || p->no_repeat_ngram_size > CAPMI_LP_NGRAM_MAX || !(p->repetition_penalty >= 1.0f) ||
        p->min_length < 0 || p->n_bad < 0 || p->n_bad > CAPMI_LP_BAD_MAX)
        return CAPMI_EINVAL;
    for (int i = 0; i < p->n_bad; ++i) {
        if (p->bad_len[i] < 1 || p->bad_len[i] > CAPMI_LP_BAD_LEN) return CAPMI_EINVAL;
        for (int k = 0; k < p->bad_len[i]; ++k)
            if (p->bad_words[i * CAPMI_LP_BAD_LEN + k] < 1) return CAPMI_EINVAL;
    }
    if (n_exempt < 0 || (n_exempt > 0 && !exempt)) return CAPMI_EINVAL;
    History h{seq, seq_ld, token, parent, W};
    if (seq) {
        if (seq_ld < t) return CAPMI_EINVAL;
    } else if (t > 0) {
        // the rows of step t > 0 are the W slots of step t - 1
        if (!token || !parent || W <= 0 || cur != W) return CAPMI_EINVAL;
    }
    if (!p->no_repeat_ngram_size && !(p->repetition_penalty > 1.0f) && !p->min_length && !p->n_bad) return 0;
    hipLaunchKernelGGL(logits_process_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, logp, ld, V1, t, L, cur, *p, h, exempt,
                       n_exempt);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
