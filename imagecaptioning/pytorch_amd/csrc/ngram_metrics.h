// The n-gram family: everything that the CIDEr-D reward (ciderd.hip), the evaluation kernels (langeval.hip: language_eval,
// eval_multi) and the training rewards (reward_mix.hip: sentence BLEU-4, self-CIDEr) share.  Key packing and the open-addressing
// document-frequency table (host twins: ciderd.py::pack_ngram / _mix64 / build_table), the two token conventions, cooking a
// caption row in LDS, the two idf rules, the clipped count walk of BLEU, the per-order cosine of two tf-idf vectors,
// bleu_scorer's score of a set of counts, and the one-wave cyclic Jacobi of self-CIDEr.  One lane per (order, start position):
// CT = NG * LMAX threads cook a row.  Every kernel of the family reads: cook my row; for each other row: stage its keys, do my
// thing; finish.
#pragma once
#include "capmi_common.h"
#include "../../../include/capmi.h"

namespace capmi {

constexpr int LMAX = 64;                    // max tokens per row: one wave holds a row
constexpr int NG = 4;                       // n-gram orders 1..4
constexpr int CT = NG * LMAX;               // one lane per (order, start position)
constexpr int NMAX = 32;                    // captions per image of a self-CIDEr matrix
static_assert(LMAX == CAPMI_WAVE, "a caption row is staged and measured by one wave");
static_assert(NMAX <= CAPMI_WAVE, "one lane per row of K");
static_assert(LMAX == CAPMI_LANGEVAL_LMAX, "capmi.h CAPMI_LANGEVAL_LMAX is the width the shared n-gram code is built for");
static_assert(NMAX == CAPMI_DIVEVAL_NMAX, "capmi.h CAPMI_DIVEVAL_NMAX is the matrix size the shared Jacobi is built for");
static_assert(NMAX == CAPMI_SELF_CIDER_NMAX, "capmi.h CAPMI_SELF_CIDER_NMAX");

// a document-frequency table has a power of two of slots (host side)
inline bool table_cap_ok(uint32_t cap) { return cap != 0 && !(cap & (cap - 1)); }

__device__ __forceinline__ uint64_t mix64(uint64_t x) {   // splitmix64 finaliser (host twin in ciderd.py)
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// tokens tok[i .. i+k] (order k+1 <= 4, ids < 65535) -> 16-bit fields of (id + 1), first token lowest; never 0
__device__ __forceinline__ uint64_t pack_ngram(const int *tok, int i, int k) {
    uint64_t key = 0;
    for (int q = 0; q <= k; ++q) key |= (uint64_t)(tok[i + q] + 1) << (16 * q);
    return key;
}

// occurrences of `key` among row[0 .. cnt) and whether position i is the first of them
__device__ __forceinline__ int ngram_tf(const uint64_t *row, int cnt, uint64_t key, int i, bool &first) {
    int tf = 0;
    for (int j = 0; j < cnt; ++j) {
        const bool same = row[j] == key;
        tf += same;
        if (same && j < i) first = false;
    }
    return tf;
}

// document frequency of `key` (0: missing).  Empty slot = key 0; cap is a power of two.
template <typename V>
__device__ __forceinline__ V df_lookup(const uint64_t *__restrict__ keys, const V *__restrict__ vals, uint32_t cap, uint64_t key) {
    uint32_t slot = (uint32_t)mix64(key) & (cap - 1);
    for (uint32_t probe = 0; probe < cap; ++probe) {
        const uint64_t k = keys[slot];
        if (k == key) return vals[slot];
        if (k == 0) return V(0);          // missing n-gram: document frequency 0
        slot = (slot + 1) & (cap - 1);
    }
    return V(0);
}

// Length of the caption in the row whose lane-th token is t (w tokens wide): the one place where a length is decided.  Whole wave.
//   KEEP_EOS false (evaluation): the tokens before the first 0.
//   KEEP_EOS true (training rewards, rewards.py:33-39 array_to_str): the row is cut AFTER its first 0, which is a word; a negative
//   token ends the row without one (the marker DeviceCiderD.pack_refs puts behind a full row of a narrower reference array).
template <bool KEEP_EOS>
__device__ __forceinline__ int caption_len(int t, int w, int lane) {
    const unsigned long long ends = __ballot(lane >= w || t <= 0);
    if (!ends) return LMAX;
    const int e = __builtin_ctzll(ends);
    if (!KEEP_EOS) return e;
    return e + (e < w && __shfl(t, e) == 0);
}

// The token conventions.  load: one token of a row (0 beyond its width); KEEP_EOS: see caption_len.
// Evaluation: int64 rows (the label file's uint32 for the training captions of sentset.hip); an id the 16-bit key fields cannot
// hold is reported in *err and ends the caption.
struct EvalTokens {
    static constexpr bool KEEP_EOS = false;
    int32_t *err;
    template <typename T>
    __device__ __forceinline__ int load(const T *row, int w, int lane) const {
        const int64_t t = lane < w ? (int64_t)row[lane] : 0;
        if (t < 0 || t >= 65535) {
            atomicOr(err, CAPMI_LANGEVAL_E_TOKEN);
            return 0;
        }
        return (int)t;
    }
};
// Training rewards: int64 (sampled rows) or int32 (packed references).
struct RewardTokens {
    static constexpr bool KEEP_EOS = true;
    template <typename T>
    __device__ __forceinline__ int load(const T *row, int w, int lane) const { return lane < w ? (int)row[lane] : 0; }
};

// occurrences of `key` among the cnt n-grams of one order of a cooked row
__device__ __forceinline__ int ngram_count(const uint64_t *row, int cnt, uint64_t key) {
    int tf = 0;
    for (int j = 0; j < cnt; ++j) tf += row[j] == key;
    return tf;
}

// A staged row (LDS): its tokens, its length, and the key of every (order k, start i) at key[k * LMAX + i], 0 past the end.
struct Row {
    uint64_t key[CT];
    int tok[LMAX];
    int len;
    __device__ __forceinline__ int count(int k, uint64_t key_h) const { return ngram_count(&key[k * LMAX], len - k, key_h); }
};

// What cooking a row leaves on lane tid = k * LMAX + i: its n-gram's key (0: none), how often the row holds it, and whether this
// is the first of those positions (exactly one lane per distinct n-gram).
struct Lane {
    uint64_t key;
    int tf;
    bool first;
    __device__ __forceinline__ static int k() { return threadIdx.x / LMAX; }
    __device__ __forceinline__ static int i() { return threadIdx.x % LMAX; }
};

// row -> R, and the calling lane's key.  Every thread of the workgroup (CT) calls it, wave 0 reads the tokens; ends with a barrier.
template <typename P, typename T>
__device__ __forceinline__ uint64_t stage_keys(Row &R, const T *row, int w, const P &tokens) {
    const int tid = threadIdx.x, k = tid / LMAX, i = tid % LMAX;
    if (__builtin_amdgcn_readfirstlane(tid) < LMAX) {     // wave 0, as a scalar branch
        const int t = tokens.load(row, w, tid);
        R.tok[tid] = t;
        const int n = caption_len<P::KEEP_EOS>(t, w, tid);
        if (tid == 0) R.len = n;
    }
    __syncthreads();
    const uint64_t key = i + k + 1 <= R.len ? pack_ngram(R.tok, i, k) : 0;
    R.key[tid] = key;
    __syncthreads();
    return key;
}

// stage_keys, then the de-duplication and the counts
template <typename P, typename T>
__device__ __forceinline__ Lane cook_row(Row &R, const T *row, int w, const P &tokens) {
    Lane c;
    c.key = stage_keys(R, row, w, tokens);
    c.first = c.key != 0;
    c.tf = c.first ? ngram_tf(&R.key[c.k() * LMAX], R.len - c.k(), c.key, c.i(), c.first) : 0;
    return c;
}

// The idf rules: two conventions on two kinds of table.  Both make an n-gram of every image weigh exactly 0, as log(n) - log(n)
// does on the host: the logarithm passed in is the host's, which need not round like the device's, and a weight of one ulp would
// turn a zero norm into a cosine of order 1.
// Evaluation table (int32 counts over the n_img images of a split): snapped where df >= n_img.
struct CorpusIdf {
    const uint64_t *keys;
    const int32_t *counts;
    uint32_t cap;
    int n_img;
    double log_n;
    __device__ __forceinline__ double operator()(uint64_t key) const {
        const int df = df_lookup(keys, counts, cap, key);
        return df >= n_img ? 0.0 : log_n - log(fmax(1.0, (double)df));
    }
};
// Training table (float64 counts, log_ref_len): as the CIDEr-D reward weighs, unsnapped ...
struct RewardIdf {
    const uint64_t *keys;
    const double *vals;
    uint32_t cap;
    double log_ref_len;
    __device__ __forceinline__ double operator()(uint64_t key) const { return log_ref_len - log(fmax(1.0, df_lookup(keys, vals, cap, key))); }
};
// ... and as self-CIDEr does: two different counts below 1e9 have logarithms at least 1e-9 apart, so a difference under 1e-12 is
// that rounding.
struct SnappedRewardIdf : RewardIdf {
    __device__ __forceinline__ double operator()(uint64_t key) const {
        const double idf = RewardIdf::operator()(key);
        return fabs(idf) < 1e-12 ? 0.0 : idf;
    }
};

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
// thread of the workgroup calls it; icontrib [CT] is LDS.
__device__ __forceinline__ int clipped_matches(int *icontrib, bool first, int tf_h, int max_tf) {
    const int tid = threadIdx.x;
    __syncthreads();
    icontrib[tid] = first ? min(tf_h, max_tf) : 0;
    __syncthreads();
    int correct = 0;
    if (tid < NG)
        for (int j = 0; j < LMAX; ++j) correct += icontrib[tid * LMAX + j];
    return correct;
}

// per-order norm of vec[CT] (0 on the lanes that hold no distinct n-gram), fixed order
__device__ __forceinline__ double order_norm(const double *vec, int k) {
    double s = 0.0;
    for (int j = 0; j < LMAX; ++j) s += vec[k * LMAX + j] * vec[k * LMAX + j];
    return sqrt(s);
}

// The four tf-idf norms of a row, to out[NG]: the body of the kernels that store them per reference / per sampled caption.
template <typename P, typename T, typename Idf>
__device__ __forceinline__ void row_norms(const T *row, int w, const P &tokens, const Idf &idf, double *out) {
    __shared__ Row R;
    __shared__ double vec[CT];
    const Lane c = cook_row(R, row, w, tokens);
    vec[threadIdx.x] = c.first ? (double)c.tf * idf(c.key) : 0.0;
    __syncthreads();
    if (threadIdx.x < NG) out[threadIdx.x] = order_norm(vec, threadIdx.x);
}

// dot product of order k: contrib[CT] holds, on the first occurrence of each n-gram of one row, the product of the two rows'
// weights of that n-gram (0 elsewhere); fixed order
__device__ __forceinline__ double order_dot(const double *contrib, int k) {
    double s = 0.0;
    for (int j = 0; j < LMAX; ++j) s += contrib[k * LMAX + j];
    return s;
}

// the cosine of one order from its dot product and the two norms; an order with a zero norm contributes 0
__device__ __forceinline__ double order_cosine(double dot, double nh, double nr) {
    return (nh != 0.0 && nr != 0.0) ? dot / (nh * nr) : 0.0;
}

// the ten counts of a caption of len words: cnt = guess 1..4, correct 1..4 (from correct[q * stride]), testlen, reflen
template <typename I, typename C>
__device__ __forceinline__ void bleu_counts(I *cnt, int len, const C *correct, int stride, int reflen) {
    for (int q = 0; q < NG; ++q) {
        cnt[q] = max(0, len - q);
        cnt[NG + q] = correct[q * stride];
    }
    cnt[8] = len;
    cnt[9] = reflen;
}

// bleu_scorer's score of one set of counts (an instance's or a corpus's): st = guess 1..4, correct 1..4, testlen, reflen
template <typename I>
__device__ __forceinline__ void bleu_of_counts(const I *st, double *out) {
    const double tiny = 1e-15, small = 1e-9;
    const double ratio = ((double)st[8] + tiny) / ((double)st[9] + small);
    const double bp = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
    double bleu = 1.0;
    for (int q = 0; q < NG; ++q) {
        bleu *= ((double)st[NG + q] + tiny) / ((double)st[q] + small);
        out[q] = pow(bleu, 1.0 / (q + 1)) * bp;
    }
}

// One wave: the eigenvalues of the symmetric A [n][n] (LDS, destroyed) by cyclic Jacobi, ascending in ev [n] (LDS).  Row-cyclic
// sweeps until the off-diagonal square sum is <= (2^-52 trace)^2, at most `sweeps`.  Lane r owns row r of the rotation.  Rotation
// (p, q) reads column p and q of every row, then writes them and (by symmetry) rows p and q; the pivot entries are lane 0's.
// Every branch is uniform: all lanes read the same LDS words.  A must be visible to the wave on entry; ev is on return.
__device__ __forceinline__ void jacobi_eigenvalues(double (*A)[NMAX + 1], int n, int lane, double *ev, int sweeps) {
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
