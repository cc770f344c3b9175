// Consensus (minimum-Bayes-risk) reranking of the n candidate captions of an image on the GPU (gfx950): keep the candidate whose
// expected utility against the other candidates is highest.  The utility is CIDEr-D, the metric training optimises, or sentence
// BLEU-4; both exactly as the rewards compute them (capmi_ciderd_score / capmi_reward_bleu4 with one reference), float64.
//
// Three launches, no atomics, no allocation, no host sync:
//   cook     one workgroup per candidate: its n-gram keys, weights (tf * idf; plain tf for BLEU), norms and length, as the cooked
//            record the CIDEr-D reward keeps of a reference (ciderd_cooked.h).  A candidate is cooked ONCE, whichever side of a
//            pair it is read on: as hypothesis and as reference a row is cut the same way (after its first 0, a full row whole).
//   pairs    one workgroup per (image, i, j): candidate i as the hypothesis against candidate j as its only reference.  The
//            hypothesis side stays in registers (one lane per n-gram position, coalesced reads of the record), the reference's
//            keys and weights are staged in LDS and searched.  B * n * n small workgroups instead of B * n that walk n references
//            each: the work of a pair is a few hundred LDS compares, so at n = 5 the walk would leave most of the chip idle and
//            at n = 32 both fill it; the record of a candidate (4.4 KB) is read n times either way and stays in L2.
//   select   one wave per image: the weights, the expected utilities, the duplicate rule, the choice.
#include "ciderd_cooked.h"

using namespace capmi;

namespace {

struct UnitIdf {         // BLEU counts n-grams: the record's weight is the plain count
    __device__ __forceinline__ double operator()(uint64_t) const { return 1.0; }
};

template <typename Idf>
__global__ __launch_bounds__(CT) void mbr_cook_kernel(const int64_t *__restrict__ hyp, int L, Idf idf, Cooked *__restrict__ out) {
    __shared__ Cooked C;
    __shared__ Row R;
    cook(R, hyp + (size_t)blockIdx.x * L, L, C, idf);
    const uint64_t *src = reinterpret_cast<const uint64_t *>(&C);
    uint64_t *dst = reinterpret_cast<uint64_t *>(out + blockIdx.x);
    for (int i = threadIdx.x; i < (int)(sizeof(Cooked) / 8); i += CT) dst[i] = src[i];
}

// blockIdx.x = (g * n + i) * n + j.  U[g][i][j], the diagonal included.
template <int KIND>
__global__ __launch_bounds__(CT) void mbr_pair_kernel(const Cooked *__restrict__ cooked, int n, double *__restrict__ U) {
    __shared__ uint64_t rkey[CT];
    __shared__ double rvec[CT];
    __shared__ uint8_t rfirst[CT];
    __shared__ double contrib[CT], score[NG];
    __shared__ int icontrib[CT], correct_s[NG];
    const int tid = threadIdx.x, k = tid / LMAX;
    const size_t hi = blockIdx.x / n;                        // the hypothesis's row g * n + i
    const size_t rj = hi / n * n + blockIdx.x % n;           // the reference's row g * n + j
    const Cooked &H = cooked[hi], &Rf = cooked[rj];
    rkey[tid] = Rf.key[tid];
    rvec[tid] = Rf.vec[tid];
    rfirst[tid] = Rf.first[tid];
    const int len_h = H.len, len_r = Rf.len;
    const bool first = H.first[tid] != 0;
    const uint64_t key = H.key[tid];
    const double vh = H.vec[tid];
    __syncthreads();
    // the reference's weight of my n-gram (0: it holds none)
    double vr = 0.0;
    if (first) {
        const int cnt = len_r - k;
        for (int j = 0; j < cnt; ++j)
            if (rfirst[k * LMAX + j] && rkey[k * LMAX + j] == key) vr = rvec[k * LMAX + j];
    }
    if (KIND == CAPMI_MBR_CIDERD) {
        contrib[tid] = first ? fmin(vh, vr) * vr : 0.0;
        __syncthreads();
        if (tid < NG) {
            double s = order_cosine(order_dot(contrib, tid), H.norm[tid], Rf.norm[tid]);
            s *= ciderd_length_term(len_h, len_r);
            score[tid] = 0.0 + s;
        }
        __syncthreads();
        if (tid == 0) {
            double m = 0.0;
            for (int q = 0; q < NG; ++q) m += score[q];
            m /= NG;
            U[blockIdx.x] = m / 1 * 10.0;                    // n_refs = 1
        }
    } else {
        const int correct = clipped_matches(icontrib, first, (int)vh, (int)vr);
        if (tid < NG) correct_s[tid] = correct;
        __syncthreads();
        if (tid == 0) {
            int cnt[10];
            bleu_counts(cnt, len_h, correct_s, 1, len_r);    // 'closest' of one reference: its length
            double b[NG];
            bleu_of_counts(cnt, b);
            U[blockIdx.x] = b[NG - 1];
        }
    }
}

// One wave per image, lane i = candidate i.  w_j = exp(seq_weight_j - max) (1 without seq_weight; the largest is exactly 1, also
// where every seq_weight is -inf); expected_i = sum_{j != i} w_j U[i][j] / sum_{j != i} w_j, j ascending, 0 where the weights of the
// others all underflow.  A candidate that repeats an earlier caption of its image (the same tokens up to and including the first
// 0) is never chosen; the choice is the lowest index with the largest expected value among the first occurrences.
__global__ __launch_bounds__(CAPMI_WAVE) void mbr_select_kernel(const double *__restrict__ U, const double *__restrict__ seq_weight,
                                                               const int64_t *__restrict__ hyp, int n, int L,
                                                               double *__restrict__ expected, int32_t *__restrict__ choice) {
    __shared__ double w[NMAX], e[NMAX];
    __shared__ int dup[NMAX];
    const int g = blockIdx.x, lane = threadIdx.x;
    if (lane < n) {
        double wl = 1.0;
        if (seq_weight) {
            const double *sw = seq_weight + (size_t)g * n;
            double mx = sw[0];
            for (int j = 1; j < n; ++j) mx = fmax(mx, sw[j]);
            wl = sw[lane] == mx ? 1.0 : exp(sw[lane] - mx);
        }
        w[lane] = wl;
        const int64_t *mine = hyp + ((size_t)g * n + lane) * L;
        int d = 0;
        for (int j = 0; j < lane && !d; ++j) {
            const int64_t *other = hyp + ((size_t)g * n + j) * L;
            int same = 1;
            for (int t = 0; t < L; ++t) {
                const int64_t a = mine[t];
                if (a != other[t]) { same = 0; break; }
                if (a == 0) break;
            }
            d = same;
        }
        dup[lane] = d;
    }
    __syncthreads();
    if (lane < n) {
        const double *u = U + ((size_t)g * n + lane) * n;
        double num = 0.0, den = 0.0;
        for (int j = 0; j < n; ++j)
            if (j != lane) {
                num += w[j] * u[j];
                den += w[j];
            }
        const double ex = den > 0.0 ? num / den : 0.0;
        e[lane] = ex;
        expected[(size_t)g * n + lane] = ex;
    }
    __syncthreads();
    if (lane == 0) {
        int best = 0;
        for (int i = 1; i < n; ++i)
            if (!dup[i] && e[i] > e[best]) best = i;
        choice[g] = best;
    }
}

}  // namespace

extern "C" int capmi_mbr_utility(const int64_t *hyp, int B, int n, int L, int kind, const uint64_t *table_keys,
                                 const double *table_vals, uint32_t table_cap, double log_ref_len, void *scratch, double *U,
                                 void *stream) {
    if (!hyp || !scratch || !U || (reinterpret_cast<uintptr_t>(scratch) & 7)) return CAPMI_EINVAL;
    if (B <= 0 || n < 2 || n > NMAX || L <= 0 || L > LMAX) return CAPMI_EINVAL;
    if (kind != CAPMI_MBR_CIDERD && kind != CAPMI_MBR_BLEU4) return CAPMI_EINVAL;
    if (kind == CAPMI_MBR_CIDERD && (!table_keys || !table_vals || !table_cap_ok(table_cap))) return CAPMI_EINVAL;
    if ((int64_t)B * n * n > INT32_MAX) return CAPMI_EINVAL;
    Cooked *cooked = reinterpret_cast<Cooked *>(scratch);
    const hipStream_t st = (hipStream_t)stream;
    if (kind == CAPMI_MBR_CIDERD) {
        hipLaunchKernelGGL(mbr_cook_kernel<RewardIdf>, dim3(B * n), dim3(CT), 0, st, hyp, L,
                           RewardIdf{table_keys, table_vals, table_cap, log_ref_len}, cooked);
        CAPMI_CHECK_LAUNCH();
        hipLaunchKernelGGL(mbr_pair_kernel<CAPMI_MBR_CIDERD>, dim3(B * n * n), dim3(CT), 0, st, cooked, n, U);
    } else {
        hipLaunchKernelGGL(mbr_cook_kernel<UnitIdf>, dim3(B * n), dim3(CT), 0, st, hyp, L, UnitIdf{}, cooked);
        CAPMI_CHECK_LAUNCH();
        hipLaunchKernelGGL(mbr_pair_kernel<CAPMI_MBR_BLEU4>, dim3(B * n * n), dim3(CT), 0, st, cooked, n, U);
    }
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_mbr_select(const double *U, const double *seq_weight, const int64_t *hyp, int B, int n, int L,
                                double *expected, int32_t *choice, void *stream) {
    if (!U || !hyp || !expected || !choice) return CAPMI_EINVAL;
    if (B <= 0 || n < 2 || n > NMAX || L <= 0 || L > LMAX) return CAPMI_EINVAL;
    hipLaunchKernelGGL(mbr_select_kernel, dim3(B), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, U, seq_weight, hyp, n, L, expected,
                       choice);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
