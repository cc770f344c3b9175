// n-gram keys and the open-addressing document-frequency table, shared by the CIDEr-D reward (ciderd.hip) and the corpus
// metrics (langeval.hip).  Host twins: ciderd.py::pack_ngram / _mix64 / build_table.
#pragma once
#include "capmi_common.h"

namespace capmi {

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

}  // namespace capmi
