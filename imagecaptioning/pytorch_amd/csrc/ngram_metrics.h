// The n-gram arithmetic that the evaluation kernels (langeval.hip: language_eval, eval_multi) and the training rewards
// (reward_mix.hip: sentence BLEU-4, self-CIDEr) share: staging a caption row in LDS under either token convention, the clipped
// count walk of BLEU, the per-order cosine of two tf-idf vectors, bleu_scorer's score of a set of counts, and the one-wave cyclic
// Jacobi of self-CIDEr.  One lane per (order, start position): CT = NG * LMAX threads cook a row, as in ciderd.hip.
#pragma once
#include "capmi_common.h"
#include "ngram_common.h"

namespace capmi {

constexpr int NM_LMAX = 64;                 // max tokens per row: one wave holds a row
constexpr int NM_NG = 4;                    // n-gram orders 1..4
constexpr int NM_CT = NM_NG * NM_LMAX;
constexpr int NM_NMAX = 32;                 // captions per image of a self-CIDEr matrix (capmi.h CAPMI_DIVEVAL_NMAX)
static_assert(NM_LMAX == CAPMI_WAVE, "a caption row is staged and measured by one wave");
static_assert(NM_NMAX <= CAPMI_WAVE, "one lane per row of K");

// Length of the caption in the row whose lane-th token is t (w tokens wide).  Whole wave.
//   KEEP_EOS false (evaluation): the tokens before the first 0.
//   KEEP_EOS true (training rewards, rewards.py:33-39 array_to_str): the row is cut AFTER its first 0, which is a word; a negative
//   token ends the row without one (the marker DeviceCiderD.pack_refs puts behind a full row of a narrower reference array).
template <bool KEEP_EOS>
__device__ __forceinline__ int caption_len(int t, int w, int lane) {
    const unsigned long long ends = __ballot(lane >= w || t <= 0);
    if (!ends) return NM_LMAX;
    const int e = __builtin_ctzll(ends);
    if (!KEEP_EOS) return e;
    return e + (e < w && __shfl(t, e) == 0);
}

// occurrences of `key` among the cnt n-grams of one order of a cooked row
__device__ __forceinline__ int ngram_count(const uint64_t *row, int cnt, uint64_t key) {
    int tf = 0;
    for (int j = 0; j < cnt; ++j) tf += row[j] == key;
    return tf;
}

// BLEU's reference length, option 'closest': the length nearest to the hypothesis's, ties to the shorter
struct ClosestLen {
    int d = 1 << 30, len = 0;
    __device__ __forceinline__ void see(int len_r, int len_h) {
        const int dl = abs(len_r - len_h);
        if (dl < d || (dl == d && len_r < len)) { d = dl; len = len_r; }
    }
};

// BLEU's clipped matches per order: thread tid offers min(tf_h, max_tf) where it holds the first occurrence of an n-gram (max_tf:
// the largest count of that n-gram in any reference walked); threads 0..NG-1 return the sum of their order, the others 0.  Every
// thread of the workgroup calls it; icontrib [NM_CT] is LDS.
__device__ __forceinline__ int clipped_matches(int *icontrib, bool first, int tf_h, int max_tf) {
    const int tid = threadIdx.x;
    __syncthreads();
    icontrib[tid] = first ? min(tf_h, max_tf) : 0;
    __syncthreads();
    int correct = 0;
    if (tid < NM_NG)
        for (int j = 0; j < NM_LMAX; ++j) correct += icontrib[tid * NM_LMAX + j];
    return correct;
}

// per-order norm of vec[NM_CT] (0 on the lanes that hold no distinct n-gram), fixed order
__device__ __forceinline__ double order_norm(const double *vec, int k) {
    double s = 0.0;
    for (int j = 0; j < NM_LMAX; ++j) s += vec[k * NM_LMAX + j] * vec[k * NM_LMAX + j];
    return sqrt(s);
}

// dot product of order k: contrib[NM_CT] holds, on the first occurrence of each n-gram of one row, the product of the two rows'
// weights of that n-gram (0 elsewhere); fixed order
__device__ __forceinline__ double order_dot(const double *contrib, int k) {
    double s = 0.0;
    for (int j = 0; j < NM_LMAX; ++j) s += contrib[k * NM_LMAX + j];
    return s;
}

// the cosine of one order from its dot product and the two norms; an order with a zero norm contributes 0
__device__ __forceinline__ double order_cosine(double dot, double nh, double nr) {
    return (nh != 0.0 && nr != 0.0) ? dot / (nh * nr) : 0.0;
}

// bleu_scorer's score of one set of counts (an instance's or a corpus's): st = guess 1..4, correct 1..4, testlen, reflen
template <typename I>
__device__ __forceinline__ void bleu_of_counts(const I *st, double *out) {
    const double tiny = 1e-15, small = 1e-9;
    const double ratio = ((double)st[8] + tiny) / ((double)st[9] + small);
    const double bp = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
    double bleu = 1.0;
    for (int q = 0; q < NM_NG; ++q) {
        bleu *= ((double)st[NM_NG + q] + tiny) / ((double)st[q] + small);
        out[q] = pow(bleu, 1.0 / (q + 1)) * bp;
    }
}

// One wave: the eigenvalues of the symmetric A [n][n] (LDS, destroyed) by cyclic Jacobi, ascending in ev [n] (LDS).  Row-cyclic
// sweeps until the off-diagonal square sum is <= (2^-52 trace)^2, at most `sweeps`.  Lane r owns row r of the rotation.  Rotation
// (p, q) reads column p and q of every row, then writes them and (by symmetry) rows p and q; the pivot entries are lane 0's.
// Every branch is uniform: all lanes read the same LDS words.  A must be visible to the wave on entry; ev is on return.
__device__ __forceinline__ void jacobi_eigenvalues(double (*A)[NM_NMAX + 1], int n, int lane, double *ev, int sweeps) {
    double trace = 0.0;
    for (int r = 0; r < n; ++r) trace += A[r][r];
    const double eps = 0x1p-52 * trace, thresh = eps * eps;
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off += A[p][q] * A[p][q];
        if (off <= thresh) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double app = A[p][p], aqq = A[q][q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                const bool mine = lane < n && lane != p && lane != q;
                const double arp = mine ? A[lane][p] : 0.0, arq = mine ? A[lane][q] : 0.0;
                __syncthreads();
                if (mine) {
                    const double np_ = c * arp - sn * arq, nq_ = sn * arp + c * arq;
                    A[lane][p] = np_; A[p][lane] = np_;
                    A[lane][q] = nq_; A[q][lane] = nq_;
                }
                if (lane == 0) {
                    A[p][p] = app - t * apq;
                    A[q][q] = aqq + t * apq;
                    A[p][q] = 0.0;
                    A[q][p] = 0.0;
                }
                __syncthreads();
            }
    }
    // ascending: the rank of an eigenvalue is the number of smaller ones (ties: the lower index first)
    if (lane < n) {
        const double x = A[lane][lane];
        int rank = 0;
        for (int r = 0; r < n; ++r) {
            const double y = A[r][r];
            rank += y < x || (y == x && r < lane);
        }
        ev[rank] = x;
    }
    __syncthreads();
}

// eval_self_cider.get_div on the ascending eigenvalues of K/10, clipped at 0; 0.0 where numpy gives NaN (the sum is 0)
__device__ __forceinline__ double self_cider_of(const double *ev, int n) {
    double sum = 0.0;
    for (int r = 0; r < n; ++r) sum += sqrt(fmax(0.0, ev[r]));
    const double top = sqrt(fmax(0.0, ev[n - 1]));
    return sum > 0.0 ? -log(top / sum) / log((double)n) : 0.0;
}

}  // namespace capmi
