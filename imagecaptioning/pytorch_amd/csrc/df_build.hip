// The CIDEr-D document-frequency table of a caption corpus on the GPU (gfx950): the device half of tools/prepro_ngrams.py
// (contract in include/capmi.h).  Keys and hash are the family's (ngram_metrics.h), so the result is the table capmi_ciderd_score,
// capmi_reward_bleu4 and capmi_self_cider_reward probe.
//
// Counting: one workgroup per image.  The image's tokens are one contiguous range of the corpus.  Every position p carries K4(p),
// the packed key of the up to four tokens that start at p and stay inside p's caption: its low 16 * n bits are the key of the
// n-gram at p, and field n - 1 is non-zero exactly when that n-gram exists.  The n-gram at p counts when no EARLIER position j of
// the image has the same low 16 * n bits -- K4(j) ^ K4(p) says so for the four orders at once.  The earlier positions pass through
// one LDS tile of DT keys (every lane reads the same word: a broadcast), so nothing bounds the size of an image and nothing but
// the order of the insertions differs from run to run.  Latency bound (a binary search over the image's caption offsets, then a
// few atomics per token); COCO's images hold about 60 tokens, a fraction of one tile.
#include "ngram_metrics.h"

using namespace capmi;

namespace {

constexpr int DT = 256;

struct DfCount {
    const void *tok;
    int64_t total_tokens;
    const int64_t *cap_off;
    int64_t n_caps;
    const int64_t *img_off;
    int n_img;
    uint64_t *keys;
    int32_t *counts;
    uint32_t cap;
    uint32_t *n_distinct;
    int32_t *err;
};

// Adds 1 to the slot of `key`; true when this call claimed the slot.
__device__ __forceinline__ bool df_count_insert(const DfCount &d, uint64_t key) {
    uint32_t slot = (uint32_t)mix64(key) & (d.cap - 1);
    for (uint32_t probe = 0; probe < d.cap; ++probe) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(d.keys + slot), 0ULL, (unsigned long long)key);
        if (prev == 0ULL || prev == key) {
            atomicAdd(d.counts + slot, 1);
            return prev == 0ULL;
        }
        slot = (slot + 1) & (d.cap - 1);
    }
    atomicOr(d.err, CAPMI_LANGEVAL_E_TABLE_FULL);
    return false;
}

// K4 of position p of an image that owns captions c0 .. c1 - 1 (offsets checked: non-decreasing, inside the corpus; p lies in
// [cap_off[c0], cap_off[c1])).
template <typename T>
__device__ __forceinline__ uint64_t key4_at(const DfCount &d, int64_t c0, int64_t c1, int64_t p) {
    int64_t lo = c0 + 1, hi = c1;                            // the first offset beyond p ends p's caption
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (d.cap_off[mid] > p) hi = mid;
        else lo = mid + 1;
    }
    const int64_t left = d.cap_off[lo] - p;
    const int n = left < NG ? (int)left : NG;
    const T *tok = static_cast<const T *>(d.tok);
    uint64_t key = 0;
    for (int q = 0; q < n; ++q) {
        int64_t t = (int64_t)tok[p + q];
        if (t < 0 || t >= 65535) {
            atomicOr(d.err, CAPMI_LANGEVAL_E_TOKEN);
            t = 0;
        }
        key |= (uint64_t)(t + 1) << (16 * q);
    }
    return key;
}

template <typename T>
__global__ __launch_bounds__(DT) void df_count_kernel(DfCount d) {
    __shared__ uint64_t tile[DT];
    __shared__ uint32_t claimed;
    const int tid = threadIdx.x;
    const int64_t c0 = d.img_off[blockIdx.x], c1 = d.img_off[blockIdx.x + 1];
    bool bad = c0 < 0 || c1 < c0 || c1 > d.n_caps || (blockIdx.x == 0 && c0 != 0) || ((int)blockIdx.x == d.n_img - 1 && c1 != d.n_caps);
    if (!bad)
        for (int64_t c = c0 + tid; c < c1; c += DT) {
            const int64_t a = d.cap_off[c], b = d.cap_off[c + 1];
            bad |= a < 0 || b < a || b > d.total_tokens;
        }
    if (tid == 0) claimed = 0;
    if (__syncthreads_or(bad)) {
        if (tid == 0) atomicOr(d.err, CAPMI_DF_E_OFFSETS);
        return;
    }
    if (c0 == c1) return;
    const int64_t t0 = d.cap_off[c0], t1 = d.cap_off[c1];

    uint32_t mine_claimed = 0;
    for (int64_t pb = t0; pb < t1; pb += DT) {
        const int64_t p = pb + tid;
        const uint64_t mine = p < t1 ? key4_at<T>(d, c0, c1, p) : 0;
        unsigned dup = 0;                                    // bit k: an earlier position starts my (k + 1)-gram
        for (int64_t jb = t0; jb <= pb; jb += DT) {
            __syncthreads();                                 // the previous tile is consumed
            tile[tid] = jb == pb ? mine : key4_at<T>(d, c0, c1, jb + tid);      // jb < pb: a whole tile of earlier positions
            __syncthreads();
            const int n = jb == pb ? tid : DT;
            if (mine)
                for (int j = 0; j < n; ++j) {
                    const uint64_t x = tile[j] ^ mine;
                    dup |= (unsigned)((x & 0xFFFFULL) == 0) | (unsigned)((x & 0xFFFFFFFFULL) == 0) << 1 |
                           (unsigned)((x & 0xFFFFFFFFFFFFULL) == 0) << 2 | (unsigned)(x == 0) << 3;
                }
        }
        for (int k = 0; k < NG; ++k) {
            const uint64_t key = k == NG - 1 ? mine : mine & ((1ULL << (16 * (k + 1))) - 1);
            if (((mine >> (16 * k)) & 0xFFFFULL) && !((dup >> k) & 1u)) mine_claimed += df_count_insert(d, key);
        }
    }
    if (mine_claimed) atomicAdd(&claimed, mine_claimed);
    __syncthreads();
    if (tid == 0 && claimed) atomicAdd(d.n_distinct, claimed);
}

constexpr int FT = 256;

// One thread per slot of the counting table (grid stride).  Every key is there once, so the thread that claims a slot of the
// image is the only one that stores its value.
__global__ __launch_bounds__(FT) void df_finalize_kernel(const uint64_t *__restrict__ count_keys, const int32_t *__restrict__ counts,
                                                        uint32_t count_cap, uint64_t *keys, double *vals, uint32_t cap, int32_t *err) {
    for (size_t s = (size_t)blockIdx.x * FT + threadIdx.x; s < count_cap; s += (size_t)gridDim.x * FT) {
        const uint64_t key = count_keys[s];
        if (key == 0) continue;
        uint32_t slot = (uint32_t)mix64(key) & (cap - 1);
        bool placed = false;
        for (uint32_t probe = 0; probe < cap && !placed; ++probe) {
            if (atomicCAS(reinterpret_cast<unsigned long long *>(keys + slot), 0ULL, (unsigned long long)key) == 0ULL) {
                vals[slot] = (double)counts[s];
                placed = true;
            }
            slot = (slot + 1) & (cap - 1);
        }
        if (!placed) atomicOr(err, CAPMI_LANGEVAL_E_TABLE_FULL);
    }
}

// off [n + 1] in host memory runs from 0 to `last` without decreasing
bool offsets_ok(const int64_t *off, int64_t n, int64_t last) {
    if (off[0] != 0 || off[n] != last) return false;
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

}  // namespace

extern "C" int capmi_df_count(const void *tok, int tok_elem, int64_t total_tokens, const int64_t *cap_off, const int64_t *cap_off_host,
                              int64_t n_caps, const int64_t *img_off, const int64_t *img_off_host, int n_img, uint64_t *table_keys,
                              int32_t *table_counts, uint32_t table_cap, uint32_t *n_distinct, int32_t *err, void *stream) {
    if (!cap_off || !img_off || !table_keys || !table_counts || !n_distinct || !err) return CAPMI_EINVAL;
    if ((tok_elem != 4 && tok_elem != 8) || total_tokens < 0 || n_caps < 0 || n_img < 0 || (!tok && total_tokens > 0)) return CAPMI_EINVAL;
    if (!table_cap_ok(table_cap)) return CAPMI_EINVAL;
    if (cap_off_host && !offsets_ok(cap_off_host, n_caps, total_tokens)) return CAPMI_EINVAL;
    if (img_off_host && !offsets_ok(img_off_host, n_img, n_caps)) return CAPMI_EINVAL;
    if (n_img == 0) return 0;
    const DfCount d{tok, total_tokens, cap_off, n_caps, img_off, n_img, table_keys, table_counts, table_cap, n_distinct, err};
    if (tok_elem == 4) hipLaunchKernelGGL(df_count_kernel<int32_t>, dim3(n_img), dim3(DT), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(df_count_kernel<int64_t>, dim3(n_img), dim3(DT), 0, (hipStream_t)stream, d);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_df_finalize(const uint64_t *count_keys, const int32_t *counts, uint32_t count_cap, uint64_t *keys, double *vals,
                                 uint32_t cap, int32_t *err, void *stream) {
    if (!count_keys || !counts || !keys || !vals || !err || !table_cap_ok(count_cap) || !table_cap_ok(cap)) return CAPMI_EINVAL;
    const uint32_t blocks = (uint32_t)(((size_t)count_cap + FT - 1) / FT);
    hipLaunchKernelGGL(df_finalize_kernel, dim3(blocks < 65536u ? blocks : 65536u), dim3(FT), 0, (hipStream_t)stream, count_keys, counts,
                       count_cap, keys, vals, cap, err);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
