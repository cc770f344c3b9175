// CIDEr-D reward on the GPU (gfx950), float64 like the upstream numpy code.
//
// Replaces the host round trip of captioning/utils/rewards.py:48-64 (D2H copy + Python string/dict
// n-gram work + pyciderevalcap.ciderD) with one launch: a workgroup per hypothesis cooks the
// hypothesis and each of its image's references in LDS (<= 4*64 n-gram positions, one lane each),
// looks the document frequency of every distinct n-gram up in an open-addressing hash table that is
// resident in HBM (built once from the pickle of scripts/prepro_ngrams.py), and evaluates the clipped
// tf-idf cosine with the Gaussian length penalty.  The arithmetic is restated from the published
// ciderD_scorer (see oracle/ciderd.py: the upstream source is absent from the reference checkout =>
// PARITY UNPINNED, anchored on the call sites and hand-derived KATs only).
//
// This kernel is latency bound (a few thousand dependent hash probes, < 0.5 MB touched): there is no
// HBM or MFMA roofline to chase, the win is removing the device->host sync from the SCST step.
//
// Keys, the token convention (cut after the first 0), the cooking of a row and the per-order norm / dot / cosine are the
// family's (ngram_metrics.h); CIDEr-D's own are the cooked blob and the length penalty (ciderd_cooked.h, shared with mbr.hip) and the
// clipped product here.
#include "ciderd_cooked.h"
#include "profile.h"

using namespace capmi;

namespace {

// References are cooked ONCE per batch (SURVEY Appendix A "refs pre-cooked per image once"): the scoring kernel below cooked
// each of an image's references again for every one of its hypotheses (300 cooks instead of 50 at bs10 x (5+1), with their
// hash probes and O(len^2) de-duplication loops).  One workgroup per (image, reference slot).
__global__ __launch_bounds__(CT) void ciderd_cook_refs_kernel(const int32_t *__restrict__ refs, const int32_t *__restrict__ n_refs,
                                                             int max_refs, int ref_w, const uint64_t *__restrict__ keys,
                                                             const double *__restrict__ vals, uint32_t cap, double log_ref_len,
                                                             Cooked *__restrict__ out) {
    __shared__ Cooked Rf;
    __shared__ Row R;
    const int img = blockIdx.x / max_refs, r = blockIdx.x % max_refs;
    if (r >= n_refs[img]) return;
    cook(R, refs + ((size_t)img * max_refs + r) * ref_w, ref_w, Rf, RewardIdf{keys, vals, cap, log_ref_len});
    const uint64_t *src = reinterpret_cast<const uint64_t *>(&Rf);
    uint64_t *dst = reinterpret_cast<uint64_t *>(out + blockIdx.x);
    for (int i = threadIdx.x; i < (int)(sizeof(Cooked) / 8); i += CT) dst[i] = src[i];
}

// COOKED: the references come pre-cooked from ciderd_cook_refs_kernel (refs / ref_w unused)
template <bool COOKED>
__global__ __launch_bounds__(CT) void ciderd_kernel(const int64_t *__restrict__ hyp, int L,
                                                   const int32_t *__restrict__ hyp_img,
                                                   const int32_t *__restrict__ refs,
                                                   const int32_t *__restrict__ n_refs, int max_refs, int ref_w,
                                                   const uint64_t *__restrict__ keys, const double *__restrict__ vals,
                                                   uint32_t cap, double log_ref_len, double *__restrict__ scores,
                                                   const Cooked *__restrict__ cooked) {
    __shared__ Cooked H, Rf;
    __shared__ Row R;
    __shared__ double contrib[CT];
    __shared__ double score[NG];
    const int h = blockIdx.x, tid = threadIdx.x;
    const int k = tid / LMAX;
    const RewardIdf idf{keys, vals, cap, log_ref_len};
    if (tid < NG) score[tid] = 0.0;
    cook(R, hyp + (size_t)h * L, L, H, idf);
    const int img = hyp_img[h];
    const int nr = n_refs[img];
    const int len_h_bi = H.len > 0 ? H.len - 1 : 0;      // upstream "length" = number of bigrams
    for (int r = 0; r < nr; ++r) {
        if (COOKED) {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(cooked + (size_t)img * max_refs + r);
            uint64_t *dst = reinterpret_cast<uint64_t *>(&Rf);
            for (int i = tid; i < (int)(sizeof(Cooked) / 8); i += CT) dst[i] = src[i];
            __syncthreads();
        } else {
            cook(R, refs + ((size_t)img * max_refs + r) * ref_w, ref_w, Rf, idf);
        }
        double cv = 0.0;
        if (H.first[tid]) {
            const uint64_t key = H.key[tid];
            const int cnt = Rf.len - k;
            double vr = 0.0;
            for (int j = 0; j < cnt; ++j)
                if (Rf.first[k * LMAX + j] && Rf.key[k * LMAX + j] == key) vr = Rf.vec[k * LMAX + j];
            const double vh = H.vec[tid];
            cv = fmin(vh, vr) * vr;
        }
        contrib[tid] = cv;
        __syncthreads();
        if (tid < NG) {
            double s = order_cosine(order_dot(contrib, tid), H.norm[tid], Rf.norm[tid]);
            const int len_r_bi = Rf.len > 0 ? Rf.len - 1 : 0;
            const double delta = (double)(len_h_bi - len_r_bi);
            s *= exp(-(delta * delta) / (2.0 * CIDERD_SIGMA * CIDERD_SIGMA));
            score[tid] += s;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double m = 0.0;
        for (int q = 0; q < NG; ++q) m += score[q];
        m /= NG;
        scores[h] = nr > 0 ? m / nr * 10.0 : 0.0;
    }
}

}  // namespace

extern "C" int capmi_ciderd_score(const int64_t *hyp, int H, int L, const int32_t *hyp_img, const int32_t *refs,
                                  const int32_t *n_refs, int max_refs, int ref_w, const uint64_t *table_keys,
                                  const double *table_vals, uint32_t table_cap, double log_ref_len, double *scores,
                                  void *stream) {
    if (!hyp || !hyp_img || !refs || !n_refs || !table_keys || !table_vals || !scores) return CAPMI_EINVAL;
    if (H <= 0 || L <= 0 || L > LMAX || ref_w <= 0 || ref_w > LMAX || max_refs <= 0) return CAPMI_EINVAL;
    if (!table_cap_ok(table_cap)) return CAPMI_EINVAL;
    hipLaunchKernelGGL(ciderd_kernel<false>, dim3(H), dim3(CT), 0, (hipStream_t)stream, hyp, L, hyp_img, refs, n_refs, max_refs,
                       ref_w, table_keys, table_vals, table_cap, log_ref_len, scores, (const Cooked *)nullptr);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_ciderd_cook_refs(const int32_t *refs, const int32_t *n_refs, int B, int max_refs, int ref_w,
                                      const uint64_t *table_keys, const double *table_vals, uint32_t table_cap,
                                      double log_ref_len, void *cooked, void *stream) {
    if (!refs || !n_refs || !table_keys || !table_vals || !cooked || B <= 0 || max_refs <= 0 || ref_w <= 0 || ref_w > LMAX)
        return CAPMI_EINVAL;
    if (!table_cap_ok(table_cap) || (reinterpret_cast<uintptr_t>(cooked) & 7)) return CAPMI_EINVAL;
    hipLaunchKernelGGL(ciderd_cook_refs_kernel, dim3(B * max_refs), dim3(CT), 0, (hipStream_t)stream, refs, n_refs, max_refs, ref_w,
                       table_keys, table_vals, table_cap, log_ref_len, reinterpret_cast<Cooked *>(cooked));
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_ciderd_score_cooked(const int64_t *hyp, int H, int L, const int32_t *hyp_img, const void *cooked,
                                         const int32_t *n_refs, int max_refs, const uint64_t *table_keys,
                                         const double *table_vals, uint32_t table_cap, double log_ref_len, double *scores,
                                         void *stream) {
    if (!hyp || !hyp_img || !cooked || !n_refs || !table_keys || !table_vals || !scores) return CAPMI_EINVAL;
    if (H <= 0 || L <= 0 || L > LMAX || max_refs <= 0) return CAPMI_EINVAL;
    if (!table_cap_ok(table_cap)) return CAPMI_EINVAL;
    hipLaunchKernelGGL(ciderd_kernel<true>, dim3(H), dim3(CT), 0, (hipStream_t)stream, hyp, L, hyp_img, (const int32_t *)nullptr,
                       n_refs, max_refs, 0, table_keys, table_vals, table_cap, log_ref_len, scores,
                       reinterpret_cast<const Cooked *>(cooked));
    CAPMI_CHECK_LAUNCH();
    return 0;
}
