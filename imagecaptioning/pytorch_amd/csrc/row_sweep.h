// What the kernels that walk a [rows, V1] float matrix one workgroup per row share (xe_loss.hip, ppo.hip, distill.hip, ensemble.hip,
// score.hip, disc.hip): the cut of a row on its own 16-byte grid, the sweep over that cut, and the fixed-order double fold of a finish kernel.
// Internal, device side.  The payloads stay with their kernels, the three running-logsumexp conventions among them.
//
// A row base does not sit on a 16-byte boundary (V1 is odd in general), so a row is cut into [0, head) scalar, [head, tail) as nv
// float4 groups and [tail, V1) scalar; head aligns the pointer the cut was made for, and every other row a sweep touches must share
// that pointer's alignment mod 16 bytes (the launchers' same_phase16, host_common.h), else the cut is made with vec == false.
#pragma once
#include "capmi_common.h"

namespace capmi {

struct RowSplit {
    int head, nv, tail, V1;
};

__device__ __forceinline__ bool same16(const void *p, const void *q) {
    return ((reinterpret_cast<uintptr_t>(p) ^ reinterpret_cast<uintptr_t>(q)) & 15) == 0;
}

// the one spelling of the alignment arithmetic; !vec: the whole row is head
__device__ __forceinline__ RowSplit row_split(const void *p, int V1, bool vec) {
    int head = V1, nv = 0;
    if (vec) {
        head = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
        head = head < V1 ? head : V1;
        nv = (V1 - head) >> 2;
    }
    return RowSplit{head, nv, head + 4 * nv, V1};
}

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// Thread tid of T: body4(v0) for the float4 groups at columns v0 = head + 4 q, q = tid, tid + T, ...; then edge1(v) for the
// thread's share of [0, head), then of [tail, V1).  Body, head, tail: the order is part of the contract, a payload that is not
// associative in float (an online logsumexp) gives other bits in any other.
template <int T, class F4, class F1>
__device__ __forceinline__ void sweep(const RowSplit &r, int tid, F4 body4, F1 edge1) {
    for (int q = tid; q < r.nv; q += T) body4(r.head + 4 * q);
    for (int v = tid; v < r.head; v += T) edge1(v);
    for (int v = r.tail + tid; v < r.V1; v += T) edge1(v);
}

// g[v] = (v == s ? c : 0) over the row: a gradient row that is zero, or the one-hot term alone (s outside [0, V1): zeros)
template <int T>
__device__ __forceinline__ void sweep_one_hot(const RowSplit &r, int tid, float *g, int64_t s, float c) {
    sweep<T>(
        r, tid,
        [&](int v0) { st4(g + v0, f32x4{v0 == s ? c : 0.f, v0 + 1 == s ? c : 0.f, v0 + 2 == s ? c : 0.f, v0 + 3 == s ? c : 0.f}); },
        [&](int v) { g[v] = v == s ? c : 0.f; });
}

// The K double sums of a T-thread workgroup, in a fixed tree (two runs are bit-equal): wave_sum_d each, lane 0 of every wave stores
// its partial sums to lds [K][T / 64], one barrier, and thread 0 alone adds the slots in ascending wave order back into s and gets
// true.  All threads of the workgroup call this.
template <int K, int T>
__device__ __forceinline__ bool fold_d(double (&s)[K], double *lds) {
    constexpr int W = T / 64;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = wave_sum_d(s[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[k * W + (tid >> 6)] = s[k];
    }
    __syncthreads();
    if (tid != 0) return false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s[k] = 0.0;
        for (int w = 0; w < W; ++w) s[k] += lds[k * W + w];
    }
    return true;
}

}  // namespace capmi
