// Sentence statistics of language_eval on the GPU (gfx950): novel_sentences, vocab_size, bad_count_rate and the mean perplexity /
// entropy of eval_utils.language_eval (eval_utils.py:27-36, 55-68, 79-80, 121), counted over token-id rows (contract and layouts in
// include/capmi.h).
//
// The training captions and the generated captions are two sets of sentences in HBM: open-addressing tables whose slot words name
// a row, so that membership is decided by the tokens and not by a hash.  One WAVE per row: lane i holds token i of a row of at
// most 64, so the row is one coalesced load, its length one ballot, its hash one butterfly sum, a token compare against another
// row one load and one ballot, and the probe sequence is uniform across the wave (lane 0 issues the atomicCAS, the others follow
// its result).  A thread per row would read 64 rows at a stride of a row per load, hash and compare token by token, and its 64
// probe chains would diverge.  All of it is latency bound; the point is that the decoded rows never leave HBM.
//
// Nothing here publishes data inside a launch: a slot word only ever names a row whose tokens were in memory before the launch
// began (the training rows are the caller's; the generated rows are stored by the launch before the inserting one).
#include "ngram_metrics.h"

using namespace capmi;

namespace {

constexpr int ST = 256;                     // threads per workgroup
constexpr int WPB = ST / CAPMI_WAVE;        // rows per workgroup: one per wave
enum { C_ROWS = 0, C_DISTINCT = 1, C_NOVEL = 2, C_FIRST = 3, C_BAD = 4 };
static_assert(C_BAD + 1 == CAPMI_SENTSET_NCOUNT, "counts [CAPMI_SENTSET_NCOUNT]");

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = CAPMI_WAVE / 2; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    return v;
}

// The hash of the sentence whose lane-th token is c (canonical: 0 from its end on, so its length is the number of non-zero lanes).
// A sum of per-position hashes: every lane contributes on its own.  Whole wave.
__device__ __forceinline__ uint64_t sentence_hash(int c, int lane, uint64_t mask) {
    const int len = __popcll(__ballot(c != 0));
    const uint64_t h = wave_sum(c != 0 ? mix64(((uint64_t)(lane + 1) << 16) | (uint64_t)(c + 1)) : 0ULL);
    return mix64(h + (uint64_t)len) & mask;
}

// canonical token of lane `lane` of a raw row: the token before the first 0, 0 from there on.  Whole wave.
template <typename T>
__device__ __forceinline__ int canonical(const T *row, int w, int lane, int32_t *err) {
    const int t = EvalTokens{err}.load(row, w, lane);
    return lane < caption_len<false>(t, w, lane) ? t : 0;
}

// how a table finds the tokens of the row a slot names
template <typename T>
struct TrainRows {
    const T *rows;
    int w;
    int32_t *err;
    __device__ __forceinline__ int operator()(uint32_t r, int lane) const { return canonical(rows + (size_t)r * w, w, lane, err); }
};
struct GenRows {
    const uint16_t *rows;
    __device__ __forceinline__ int operator()(uint32_t r, int lane) const { return rows[(size_t)r * LMAX + lane]; }
};

__device__ __forceinline__ uint32_t tag_of(uint64_t w) { return (uint32_t)(w >> 32); }

// Insert the sentence (hash h, lane-th token c) that row `row` holds.  1: this wave claimed an empty slot, the slot now names
// `row`; 0: the sentence was there (or a twin in flight claimed it first); -1: no slot left.  Whole wave, uniform result.
// The race of equal sentences: each of their waves runs the same probe sequence, and the atomicCAS on a slot returns 0 to exactly
// one wave per slot.  Whoever loses at a slot holds the winner's word, reads the row it names and, finding its own tokens there,
// leaves; finding others, probes on.  So one of the twins counts, whichever.
template <typename Rows>
__device__ __forceinline__ int set_insert(uint64_t *table, uint32_t cap, uint64_t h, uint32_t row, int c, int lane, const Rows &rows) {
    const unsigned long long word = (h & 0xffffffff00000000ULL) | (unsigned long long)(row + 1u);
    uint32_t slot = (uint32_t)h & (cap - 1);
    for (uint32_t probe = 0; probe < cap; ++probe) {
        unsigned long long prev = 0;
        if (lane == 0) prev = atomicCAS(reinterpret_cast<unsigned long long *>(table + slot), 0ULL, word);
        prev = __shfl(prev, 0);
        if (prev == 0ULL) return 1;
        if (tag_of(prev) == tag_of(word) && !__ballot(rows((uint32_t)prev - 1u, lane) != c)) return 0;
        slot = (slot + 1) & (cap - 1);
    }
    return -1;
}

// Is the sentence in a table that no launch in flight writes?  Whole wave, uniform result.
template <typename Rows>
__device__ __forceinline__ bool set_contains(const uint64_t *table, uint32_t cap, uint64_t h, int c, int lane, const Rows &rows) {
    uint32_t slot = (uint32_t)h & (cap - 1);
    for (uint32_t probe = 0; probe < cap; ++probe) {
        const uint64_t w = table[slot];
        if (w == 0) return false;
        if (tag_of(w) == tag_of(h) && !__ballot(rows((uint32_t)w - 1u, lane) != c)) return true;
        slot = (slot + 1) & (cap - 1);
    }
    return false;
}

__device__ __forceinline__ bool holds(int c, int unk_id) { return unk_id > 0 && __ballot(c == unk_id) != 0ULL; }

// One wave per training row.
template <typename T>
__global__ __launch_bounds__(ST) void sentset_build_kernel(capmi_sentset s) {
    const int lane = threadIdx.x % CAPMI_WAVE;
    const int64_t row = (int64_t)blockIdx.x * WPB + threadIdx.x / CAPMI_WAVE;
    if (row >= s.n_train) return;                            // uniform across the wave
    const TrainRows<T> rows{static_cast<const T *>(s.train_rows), s.train_w, s.err};
    const int c = rows((uint32_t)row, lane);
    if (holds(c, s.unk_id)) return;                          // the reference's raw training strings never spell UNK
    const uint64_t h = sentence_hash(c, lane, s.hash_mask);
    if (set_insert(s.train_table, s.train_cap, h, (uint32_t)row, c, lane, rows) < 0 && lane == 0)
        atomicOr(s.err, CAPMI_LANGEVAL_E_TABLE_FULL);
}

// One wave per generated row: the canonical row to gen_rows, its tokens into the bitmap.
__global__ __launch_bounds__(ST) void sentset_stage_kernel(capmi_sentset s, const int64_t *__restrict__ seqs, int n_rows, int L, int base) {
    const int lane = threadIdx.x % CAPMI_WAVE;
    const int r = blockIdx.x * WPB + threadIdx.x / CAPMI_WAVE;
    if (r >= n_rows) return;
    int c = canonical(seqs + (size_t)r * L, L, lane, s.err);
    if (c >= s.V1) {                                         // outside the bitmap: reported, never stored
        atomicOr(s.err, CAPMI_LANGEVAL_E_TOKEN);
        c = 0;
    }
    if (__ballot(c == 0) & ((1ULL << lane) - 1ULL)) c = 0;   // a refused token ends the sentence: the stored row stays canonical
    s.gen_rows[(size_t)(base + r) * LMAX + lane] = (uint16_t)c;
    if (c > 0) {
        uint32_t *word = s.vocab_bits + (c >> 5);
        const uint32_t bit = 1u << (c & 31);
        if (!(*word & bit)) atomicOr(word, bit);             // bits are only ever set: a stale read costs one redundant atomic
    }
}

// One wave per generated row, after sentset_stage_kernel.
template <typename T>
__global__ __launch_bounds__(ST) void sentset_insert_kernel(capmi_sentset s, int n_rows, int base) {
    const int lane = threadIdx.x % CAPMI_WAVE;
    const int r = blockIdx.x * WPB + threadIdx.x / CAPMI_WAVE;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long *>(s.counts + C_ROWS), (unsigned long long)n_rows);
    if (r >= n_rows) return;
    const GenRows gen{s.gen_rows};
    const uint32_t row = (uint32_t)(base + r);
    const int c = gen(row, lane);
    const uint64_t h = sentence_hash(c, lane, s.hash_mask);
    const int got = set_insert(s.gen_table, s.gen_cap, h, row, c, lane, gen);
    if (got < 0 && lane == 0) atomicOr(s.err, CAPMI_LANGEVAL_E_TABLE_FULL);
    if (got != 1) return;
    const TrainRows<T> train{static_cast<const T *>(s.train_rows), s.train_w, s.err};
    const bool novel = holds(c, s.unk_id) || !set_contains(s.train_table, s.train_cap, h, c, lane, train);
    if (lane == 0) {
        atomicAdd(reinterpret_cast<unsigned long long *>(s.counts + C_DISTINCT), 1ULL);
        if (novel) atomicAdd(reinterpret_cast<unsigned long long *>(s.counts + C_NOVEL), 1ULL);
    }
}

// One workgroup: the single-caption pass.  Thread t takes rows t, t + ST, ...; thread 0 adds the ST partial sums in index order.
__global__ __launch_bounds__(ST) void sentset_first_kernel(capmi_sentset s, const int64_t *__restrict__ seq, int n_rows, int L,
                                                          const float *__restrict__ perplexity, const float *__restrict__ entropy) {
    __shared__ double sp[ST], se[ST];
    __shared__ unsigned sb[ST];
    const int tid = threadIdx.x;
    double p = 0.0, e = 0.0;
    unsigned bad = 0;
    for (int r = tid; r < n_rows; r += ST) {
        const int64_t *row = seq + (size_t)r * L;
        int64_t last = 0;
        for (int j = 0; j < L; ++j) {
            const int64_t t = row[j];
            if (t < 0 || t >= 65535) {
                atomicOr(s.err, CAPMI_LANGEVAL_E_TOKEN);
                break;
            }
            if (t == 0) break;
            last = t;
        }
        if (last != 0)                                       // an empty caption ends in no word
            for (int q = 0; q < s.n_bad; ++q)
                if (s.bad[q] == last) { ++bad; break; }
        p += (double)perplexity[r];
        e += (double)entropy[r];
    }
    sp[tid] = p;
    se[tid] = e;
    sb[tid] = bad;
    __syncthreads();
    if (tid == 0) {
        double tp = 0.0, te = 0.0;
        unsigned long long tb = 0;
        for (int j = 0; j < ST; ++j) { tp += sp[j]; te += se[j]; tb += sb[j]; }
        s.sums[0] += tp;                                     // launches of one stream: one writer at a time
        s.sums[1] += te;
        s.counts[C_FIRST] += (uint64_t)n_rows;
        s.counts[C_BAD] += tb;
    }
}

// One workgroup: the record the host reads.
__global__ __launch_bounds__(ST) void sentset_reduce_kernel(capmi_sentset s, double *__restrict__ out) {
    __shared__ unsigned words;
    if (threadIdx.x == 0) words = 0;
    __syncthreads();
    unsigned bits = 0;
    for (int w = threadIdx.x; w < (s.V1 + 31) / 32; w += ST) bits += __popc(s.vocab_bits[w]);
    atomicAdd(&words, bits);                                 // integers: any order
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 0; q < CAPMI_SENTSET_NCOUNT; ++q) out[q] = (double)s.counts[q];
        out[5] = (double)words;
        out[6] = s.sums[0];
        out[7] = s.sums[1];
        out[8] = (double)*s.err;
    }
}
static_assert(CAPMI_SENTSET_NOUT == 9, "out [CAPMI_SENTSET_NOUT]");

bool sentset_valid(const capmi_sentset *s) {
    if (!s || !s->train_table || !s->gen_table || !s->vocab_bits || !s->counts || !s->sums || !s->err) return false;
    if (s->n_train < 0 || s->gen_capacity < 0 || s->n_bad < 0 || s->V1 < 1 || s->V1 > 65536) return false;
    if (s->n_train > 0 && (!s->train_rows || s->train_w < 1 || s->train_w > LMAX)) return false;
    if (s->train_elem != 4 && s->train_elem != 8) return false;
    if (s->gen_capacity > 0 && !s->gen_rows) return false;
    if (s->n_bad > 0 && !s->bad) return false;
    return table_cap_ok(s->train_cap) && table_cap_ok(s->gen_cap);
}

inline int blocks_for(int rows) { return (rows + WPB - 1) / WPB; }

}  // namespace

extern "C" int capmi_sentset_build(const capmi_sentset *s, void *stream) {
    if (!sentset_valid(s)) return CAPMI_EINVAL;
    if (s->n_train == 0) return 0;
    if (s->train_elem == 8)
        hipLaunchKernelGGL(sentset_build_kernel<int64_t>, dim3(blocks_for(s->n_train)), dim3(ST), 0, (hipStream_t)stream, *s);
    else
        hipLaunchKernelGGL(sentset_build_kernel<uint32_t>, dim3(blocks_for(s->n_train)), dim3(ST), 0, (hipStream_t)stream, *s);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_sentset_add(const capmi_sentset *s, const int64_t *seqs, int rows, int L, int base_row, void *stream) {
    if (!sentset_valid(s) || rows < 0 || L < 1 || L > LMAX || base_row < 0) return CAPMI_EINVAL;
    if (rows == 0) return 0;
    if (!seqs || (int64_t)base_row + rows > s->gen_capacity) return CAPMI_EINVAL;
    hipLaunchKernelGGL(sentset_stage_kernel, dim3(blocks_for(rows)), dim3(ST), 0, (hipStream_t)stream, *s, seqs, rows, L, base_row);
    CAPMI_CHECK_LAUNCH();
    if (s->train_elem == 8)
        hipLaunchKernelGGL(sentset_insert_kernel<int64_t>, dim3(blocks_for(rows)), dim3(ST), 0, (hipStream_t)stream, *s, rows, base_row);
    else
        hipLaunchKernelGGL(sentset_insert_kernel<uint32_t>, dim3(blocks_for(rows)), dim3(ST), 0, (hipStream_t)stream, *s, rows, base_row);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_sentset_add_first(const capmi_sentset *s, const int64_t *seq, int rows, int L, const float *perplexity,
                                       const float *entropy, void *stream) {
    if (!sentset_valid(s) || rows < 0 || L < 1 || L > LMAX) return CAPMI_EINVAL;
    if (rows == 0) return 0;
    if (!seq || !perplexity || !entropy) return CAPMI_EINVAL;
    hipLaunchKernelGGL(sentset_first_kernel, dim3(1), dim3(ST), 0, (hipStream_t)stream, *s, seq, rows, L, perplexity, entropy);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_sentset_reduce(const capmi_sentset *s, double *out, void *stream) {
    if (!sentset_valid(s) || !out) return CAPMI_EINVAL;
    hipLaunchKernelGGL(sentset_reduce_kernel, dim3(1), dim3(ST), 0, (hipStream_t)stream, *s, out);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
