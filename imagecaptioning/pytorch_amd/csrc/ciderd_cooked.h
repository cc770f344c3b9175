// The cooked record of a caption row, shared by the CIDEr-D reward (ciderd.hip: references cooked once per batch) and the
// consensus reranking (mbr.hip: every candidate cooked once, then read as hypothesis and as reference): the key of every n-gram
// position, its weight on the first occurrence of each distinct n-gram, the four norms and the length.
#pragma once
#include "ngram_metrics.h"

namespace capmi {

constexpr double CIDERD_SIGMA = 6.0;

struct Cooked {
    uint64_t key[CT];
    double vec[CT];      // tf * idf on the FIRST occurrence of each distinct n-gram, else 0
    uint8_t first[CT];
    double norm[NG];
    int len;             // tokens kept (up to and including the first 0)
};

static_assert(sizeof(Cooked) == CAPMI_CIDERD_COOKED_BYTES, "capmi.h CAPMI_CIDERD_COOKED_BYTES must equal sizeof(Cooked)");

// all CT threads participate.  row: int64 (hypotheses) or int32 (packed references), w tokens wide; R is scratch.
template <typename T, typename Idf>
__device__ void cook(Row &R, const T *row, int w, Cooked &c, const Idf &idf) {
    const int tid = threadIdx.x;
    const Lane l = cook_row(R, row, w, RewardTokens());
    double v = 0.0;
    if (l.first) v = (double)l.tf * idf(l.key);
    c.key[tid] = l.key;
    c.vec[tid] = v;
    c.first[tid] = l.first ? 1 : 0;
    if (tid == 0) c.len = R.len;
    __syncthreads();
    if (tid < NG) c.norm[tid] = order_norm(c.vec, tid);
    __syncthreads();
}

// The Gaussian length term of one (hypothesis, reference) pair; upstream's "length" is the number of bigrams
__device__ __forceinline__ double ciderd_length_term(int len_h, int len_r) {
    const int len_h_bi = len_h > 0 ? len_h - 1 : 0, len_r_bi = len_r > 0 ? len_r - 1 : 0;
    const double delta = (double)(len_h_bi - len_r_bi);
    return exp(-(delta * delta) / (2.0 * CIDERD_SIGMA * CIDERD_SIGMA));
}

}  // namespace capmi
