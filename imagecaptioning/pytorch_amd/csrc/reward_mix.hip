// Sentence BLEU-4 and self-CIDEr as training rewards on the GPU (gfx950): bleu_reward_weight (reference rewards.py:68-74, 105-112)
// and self_cider_reward_weight (rewards.py:116-136, losses.py:175-182), float64 like the CIDEr-D reward beside them.
//
// The n-gram arithmetic is the evaluation's (ngram_metrics.h, shared with langeval.hip); what differs is the convention of the
// call site.  Tokens: a row is cut AFTER its first 0 (array_to_str keeps the 0 as a word), a negative token is pack_refs' marker
// behind a full row of a narrower reference array.  Document frequencies of self-CIDEr: the training table of the CIDEr-D reward
// (float64 counts, log_ref_len), weight of an n-gram = tf * (log_ref_len - log(max(1, df))).
//
// Like ciderd.hip this is latency bound (a few LDS compares and hash probes per caption): the point is that the sampled rows
// never leave HBM, that the reward mix costs no launch of its own, and that a step with these rewards can be captured.
#include "capmi_common.h"
#include "ngram_common.h"
#include "ngram_metrics.h"
#include "../../../include/capmi.h"

namespace {

using capmi::bleu_of_counts;
using capmi::clipped_matches;
using capmi::ClosestLen;
using capmi::df_lookup;
using capmi::jacobi_eigenvalues;
using capmi::ngram_count;
using capmi::ngram_tf;
using capmi::order_cosine;
using capmi::order_dot;
using capmi::order_norm;
using capmi::pack_ngram;
using capmi::self_cider_of;

constexpr int LMAX = capmi::NM_LMAX;
constexpr int NG = capmi::NM_NG;
constexpr int CT = capmi::NM_CT;            // one lane per (order, start position)
constexpr int NMAX = capmi::NM_NMAX;
static_assert(NMAX == CAPMI_SELF_CIDER_NMAX, "capmi.h CAPMI_SELF_CIDER_NMAX");

// row -> tok[LMAX], *len (LDS) under the training convention; every thread of the workgroup calls it, wave 0 works; ends with a
// barrier.  T: int64 (sampled rows) or int32 (packed references).
template <typename T>
__device__ __forceinline__ void stage_reward_row(const T *row, int w, int *tok, int *len) {
    if (threadIdx.x < LMAX) {
        const int lane = threadIdx.x;
        const int t = lane < w ? (int)row[lane] : 0;
        tok[lane] = t;
        const int n = capmi::caption_len<true>(t, w, lane);
        if (lane == 0) *len = n;
    }
    __syncthreads();
}

// This file is built with -ffp-contract=off (build.py EXTRA_FLAGS): the call site's arithmetic must round like the reference's
// separate numpy / torch operations -- cider_reward_weight * cider + bleu_reward_weight * bleu is two rounded products and a
// rounded sum, `scores += w * x` a rounded product and a rounded sum -- and under -ffp-contract=fast the backend fuses a product
// into a sum whatever a pragma says.

// One workgroup per hypothesis row: the row is cooked once, the image's references are walked once; every hypothesis n-gram
// keeps the largest count a reference holds of it, and the closest reference length is tracked beside.
// out[h] = cw * base[h] + bw * bleu4 (base may be out: each entry is read and written by the same thread), or bw * bleu4.
// stats [H, 10] (when given) = guess 1..4, correct 1..4, testlen, reflen.
__global__ __launch_bounds__(CT) void reward_bleu4_kernel(const int64_t *__restrict__ hyp, int L, const int32_t *__restrict__ hyp_img,
                                                         const int32_t *__restrict__ refs, const int32_t *__restrict__ n_refs, int B,
                                                         int max_refs, int ref_w, const double *base, double cw, double bw,
                                                         double *out, int32_t *__restrict__ stats) {
    __shared__ int tok_h[LMAX], tok_r[LMAX], len_s[2], icontrib[CT], correct_s[NG];
    __shared__ uint64_t key_h[CT], key_r[CT];
    const int h = blockIdx.x, tid = threadIdx.x, k = tid / LMAX, i = tid % LMAX;

    stage_reward_row(hyp + (size_t)h * L, L, tok_h, &len_s[0]);
    const int len_h = len_s[0];
    const bool valid = i + k + 1 <= len_h;
    const uint64_t key = valid ? pack_ngram(tok_h, i, k) : 0;
    key_h[tid] = key;
    __syncthreads();
    bool first = valid;
    int tf_h = 0;
    if (valid) tf_h = ngram_tf(&key_h[k * LMAX], len_h - k, key, i, first);

    const int img = hyp_img[h];
    const int nr = (img >= 0 && img < B) ? min(n_refs[img], max_refs) : 0;
    int max_tf = 0;
    ClosestLen closest;
    for (int r = 0; r < nr; ++r) {
        __syncthreads();                                     // tok_r / key_r of the previous reference are consumed
        stage_reward_row(refs + ((size_t)img * max_refs + r) * ref_w, ref_w, tok_r, &len_s[1]);
        const int len_r = len_s[1];
        key_r[tid] = i + k + 1 <= len_r ? pack_ngram(tok_r, i, k) : 0;
        __syncthreads();
        const int tf_r = first ? ngram_count(&key_r[k * LMAX], len_r - k, key) : 0;
        max_tf = max(max_tf, tf_r);
        closest.see(len_r, len_h);
    }
    const int correct = clipped_matches(icontrib, first, tf_h, max_tf);
    if (tid < NG) correct_s[tid] = correct;
    __syncthreads();
    if (tid == 0) {
        int cnt[10];
        for (int q = 0; q < NG; ++q) { cnt[q] = max(0, len_h - q); cnt[NG + q] = correct_s[q]; }
        cnt[8] = len_h;
        cnt[9] = closest.len;
        double b[NG];
        bleu_of_counts(cnt, b);
        if (stats)
            for (int q = 0; q < 10; ++q) stats[(size_t)h * 10 + q] = cnt[q];
        out[h] = base ? cw * base[h] + bw * b[NG - 1] : bw * b[NG - 1];
    }
}

// One workgroup per sampled row (image g, slot s): its four tf-idf norms, and the per-order dot products with the rows of slots
// o >= s of the same image (the n-gram is the same on both sides, so is its idf).  norm [B * n, 4], dots [B * n, n, 4] (o >= s).
__global__ __launch_bounds__(CT) void self_cider_walk_kernel(const int64_t *__restrict__ hyp, int n, int L,
                                                            const uint64_t *__restrict__ keys, const double *__restrict__ vals,
                                                            uint32_t cap, double log_ref_len, double *__restrict__ norm,
                                                            double *__restrict__ dots) {
    __shared__ int tok_h[LMAX], tok_r[LMAX], len_s[2];
    __shared__ uint64_t key_h[CT], key_r[CT];
    __shared__ double contrib[CT];
    const int tid = threadIdx.x, k = tid / LMAX, i = tid % LMAX, g = blockIdx.x / n, s = blockIdx.x % n;
    const int64_t *rows = hyp + (size_t)g * n * L;

    stage_reward_row(rows + (size_t)s * L, L, tok_h, &len_s[0]);
    const int len_h = len_s[0];
    const bool valid = i + k + 1 <= len_h;
    const uint64_t key = valid ? pack_ngram(tok_h, i, k) : 0;
    key_h[tid] = key;
    __syncthreads();
    bool first = valid;
    int tf_h = 0;
    if (valid) tf_h = ngram_tf(&key_h[k * LMAX], len_h - k, key, i, first);
    // an n-gram of every image weighs exactly 0, as log(ref_len) - log(ref_len) does on the host: log_ref_len is the host's
    // logarithm, which need not round like the device's, and a weight of one ulp would turn a zero norm into a cosine of order 1.
    // Two different counts below 1e9 have logarithms at least 1e-9 apart, so a difference under 1e-12 is that rounding.
    double idf = first ? log_ref_len - log(fmax(1.0, df_lookup(keys, vals, cap, key))) : 0.0;
    if (fabs(idf) < 1e-12) idf = 0.0;
    const double vh = (double)tf_h * idf;
    contrib[tid] = first ? vh : 0.0;
    __syncthreads();
    if (tid < NG) norm[(size_t)blockIdx.x * NG + tid] = order_norm(contrib, tid);

    for (int o = s; o < n; ++o) {
        __syncthreads();                                     // tok_r / key_r / contrib of the previous caption are consumed
        stage_reward_row(rows + (size_t)o * L, L, tok_r, &len_s[1]);
        const int len_r = len_s[1];
        key_r[tid] = i + k + 1 <= len_r ? pack_ngram(tok_r, i, k) : 0;
        __syncthreads();
        const int tf_r = first ? ngram_count(&key_r[k * LMAX], len_r - k, key) : 0;
        contrib[tid] = first ? vh * ((double)tf_r * idf) : 0.0;
        __syncthreads();
        if (tid < NG) dots[((size_t)blockIdx.x * n + o) * NG + tid] = order_dot(contrib, tid);
    }
}

// One wave per image: K from the dot products and norms (upper triangle, mirrored: exactly symmetric), the eigenvalues of K/10
// by the cyclic Jacobi of the evaluation, the score.  K_out [B, n, n] and eig_out [B, n] are written when given.
__global__ __launch_bounds__(CAPMI_WAVE) void self_cider_finish_kernel(const double *__restrict__ norm, const double *__restrict__ dots,
                                                                      int n, double *__restrict__ out, double *__restrict__ K_out,
                                                                      double *__restrict__ eig_out) {
    __shared__ double A[NMAX][NMAX + 1], ev[NMAX];
    const int g = blockIdx.x, lane = threadIdx.x;
    for (int idx = lane; idx < n * n; idx += CAPMI_WAVE) {
        const int s = idx / n, o = idx % n;
        if (s > o) continue;
        const size_t rs = (size_t)g * n + s, ro = (size_t)g * n + o;
        double m = 0.0;
        for (int q = 0; q < NG; ++q) m += order_cosine(dots[(rs * n + o) * NG + q], norm[rs * NG + q], norm[ro * NG + q]);
        const double v = m / NG * 10.0;
        A[s][o] = v / 10.0;
        A[o][s] = v / 10.0;
        if (K_out) {
            K_out[rs * n + o] = v;
            K_out[ro * n + s] = v;
        }
    }
    __syncthreads();
    jacobi_eigenvalues(A, n, lane, ev, CAPMI_DIVEVAL_SWEEPS);
    if (eig_out && lane < n) eig_out[(size_t)g * n + lane] = ev[lane];
    if (lane == 0) out[g] = self_cider_of(ev, n);            // every weight zero: 0.0, not NaN
}

// One workgroup.  reward [N] = the scores as float32 (what StructureLosses reports), adv [N] = new_self_critical's leave-one-out
// advantage plus add_w * add[image], in the reference's float32 order of operations (losses.py:175-182).
__global__ void nsc_advantage_kernel(const double *__restrict__ scores, const double *__restrict__ add, float add_w, int N, int n,
                                     float *__restrict__ reward, float *__restrict__ adv) {
    for (int r = threadIdx.x; r < N; r += blockDim.x) {
        const int g = r / n;
        float sum = 0.f;
        for (int j = 0; j < n; ++j) sum += (float)scores[(size_t)g * n + j];
        const float s = (float)scores[r];
        float a = s - (sum - s) / (float)(n - 1);
        if (add) a = a + add_w * (float)add[g];
        reward[r] = s;
        adv[r] = a;
    }
}

bool table_ok(const uint64_t *keys, const double *vals, uint32_t cap) { return keys && vals && cap != 0 && !(cap & (cap - 1)); }

}  // namespace

extern "C" int capmi_reward_bleu4(const int64_t *hyp, int H, int L, const int32_t *hyp_img, const int32_t *refs,
                                  const int32_t *n_refs, int B, int max_refs, int ref_w, const double *base, double cw, double bw,
                                  double *scores, int32_t *stats, void *stream) {
    if (!hyp || !hyp_img || !refs || !n_refs || !scores) return CAPMI_EINVAL;
    if (H <= 0 || L <= 0 || L > LMAX || ref_w <= 0 || ref_w > LMAX || max_refs <= 0 || B <= 0) return CAPMI_EINVAL;
    hipLaunchKernelGGL(reward_bleu4_kernel, dim3(H), dim3(CT), 0, (hipStream_t)stream, hyp, L, hyp_img, refs, n_refs, B, max_refs,
                       ref_w, base, cw, bw, scores, stats);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_self_cider_reward(const int64_t *hyp, int B, int n, int L, const uint64_t *table_keys, const double *table_vals,
                                       uint32_t table_cap, double log_ref_len, double *norm, double *dots, double *scores, double *K,
                                       double *eig, void *stream) {
    if (!hyp || !norm || !dots || !scores || !table_ok(table_keys, table_vals, table_cap)) return CAPMI_EINVAL;
    if (B <= 0 || n < 2 || n > NMAX || L <= 0 || L > LMAX) return CAPMI_EINVAL;
    hipLaunchKernelGGL(self_cider_walk_kernel, dim3(B * n), dim3(CT), 0, (hipStream_t)stream, hyp, n, L, table_keys, table_vals,
                       table_cap, log_ref_len, norm, dots);
    CAPMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(self_cider_finish_kernel, dim3(B), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, norm, dots, n, scores, K, eig);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_nsc_advantage(const double *scores, const double *add, double add_w, int N, int n, float *reward, float *adv,
                                   void *stream) {
    if (!scores || !reward || !adv || N <= 0 || n < 2 || N % n) return CAPMI_EINVAL;
    hipLaunchKernelGGL(nsc_advantage_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scores, add, (float)add_w, N, n, reward, adv);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
