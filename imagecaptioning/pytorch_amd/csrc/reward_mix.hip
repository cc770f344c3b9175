// Sentence BLEU-4 and self-CIDEr as training rewards on the GPU (gfx950): bleu_reward_weight (reference rewards.py:68-74, 105-112)
// and self_cider_reward_weight (rewards.py:116-136, losses.py:175-182), float64 like the CIDEr-D reward beside them.
//
// Cooking a row, staging the rows it is walked against and the n-gram arithmetic are the family's (ngram_metrics.h); this file
// keeps the walks' per-pair logic, the reward mix and the advantage.  What differs from the evaluation is the convention of the
// call site, both named there.  Tokens (RewardTokens): a row is cut AFTER its first 0 (array_to_str keeps the 0 as a word), a
// negative token is pack_refs' marker behind a full row of a narrower reference array.  Document frequencies of self-CIDEr
// (SnappedRewardIdf): the training table of the CIDEr-D reward (float64 counts, log_ref_len), weight of an n-gram =
// tf * (log_ref_len - log(max(1, df))).
//
// Like ciderd.hip this is latency bound (a few LDS compares and hash probes per caption): the point is that the sampled rows
// never leave HBM, that the reward mix costs no launch of its own, and that a step with these rewards can be captured.
#include "ngram_metrics.h"

using namespace capmi;

namespace {

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
    __shared__ Row Hr, Rr;
    __shared__ int icontrib[CT], correct_s[NG];
    const int h = blockIdx.x, tid = threadIdx.x;
    const Lane c = cook_row(Hr, hyp + (size_t)h * L, L, RewardTokens());
    const int len_h = Hr.len;

    const int img = hyp_img[h];
    const int nr = (img >= 0 && img < B) ? min(n_refs[img], max_refs) : 0;
    int max_tf = 0;
    ClosestLen closest;
    for (int r = 0; r < nr; ++r) {
        __syncthreads();                                     // Rr of the previous reference is consumed
        stage_keys(Rr, refs + ((size_t)img * max_refs + r) * ref_w, ref_w, RewardTokens());
        const int tf_r = c.first ? Rr.count(c.k(), c.key) : 0;
        max_tf = max(max_tf, tf_r);
        closest.see(Rr.len, len_h);
    }
    const int correct = clipped_matches(icontrib, c.first, c.tf, max_tf);
    if (tid < NG) correct_s[tid] = correct;
    __syncthreads();
    if (tid == 0) {
        int cnt[10];
        bleu_counts(cnt, len_h, correct_s, 1, closest.len);
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
    __shared__ Row Hr, Rr;
    __shared__ double contrib[CT];
    const int tid = threadIdx.x, g = blockIdx.x / n, s = blockIdx.x % n;
    const int64_t *rows = hyp + (size_t)g * n * L;

    const Lane c = cook_row(Hr, rows + (size_t)s * L, L, RewardTokens());
    const double idf = c.first ? SnappedRewardIdf{{keys, vals, cap, log_ref_len}}(c.key) : 0.0;
    const double vh = (double)c.tf * idf;
    contrib[tid] = c.first ? vh : 0.0;
    __syncthreads();
    if (tid < NG) norm[(size_t)blockIdx.x * NG + tid] = order_norm(contrib, tid);

    for (int o = s; o < n; ++o) {
        __syncthreads();                                     // Rr / contrib of the previous caption are consumed
        stage_keys(Rr, rows + (size_t)o * L, L, RewardTokens());
        const int tf_r = c.first ? Rr.count(c.k(), c.key) : 0;
        contrib[tid] = c.first ? vh * ((double)tf_r * idf) : 0.0;
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
    if (!hyp || !norm || !dots || !scores || !table_keys || !table_vals || !table_cap_ok(table_cap)) return CAPMI_EINVAL;
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
