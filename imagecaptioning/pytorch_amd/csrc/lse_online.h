// The running logsumexp of the kernels that normalise M rows at once and then combine them column by column (ensemble.hip, disc.hip):
// per thread M pairs (max, sum exp(x - max)), folded over the workgroup in one barrier pair for all M.  Internal, device side.
// The convention (row_sweep.h names three): base 0 while the max is -inf, a NaN leaves the max alone and reaches the sum.
#pragma once
#include "capmi_common.h"

namespace capmi {

// (max, sum exp(x - max)) folded with x.  A NaN x leaves the max alone and reaches the sum; while the max is still -inf the
// sum stays 0 without forming -inf - -inf.
__device__ __forceinline__ void online1(float &m, float &s, float x) {
    const float nm = fmaxf(m, x);
    const float base = nm == -INFINITY ? 0.f : nm;
    s = s * __expf(m - base) + __expf(x - base);
    m = nm;
}
__device__ __forceinline__ void online4(float &m, float &s, f32x4 x) {
    const float nm = fmaxf(m, fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)));
    const float base = nm == -INFINITY ? 0.f : nm;
    s = s * __expf(m - base) + ((__expf(x.x - base) + __expf(x.y - base)) + (__expf(x.z - base) + __expf(x.w - base)));
    m = nm;
}

// block-wide max of M values at once (one barrier pair instead of M), then the rescaled sums likewise; W waves per workgroup
template <int M, int W>
__device__ __forceinline__ void block_lse(float (&m)[M], float (&s)[M], float *scratch /* [2][M][W] */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const float wm = wave_max(m[i]);
        if (lane == 0) scratch[i * W + wid] = wm;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < M; ++i) {
        float r = scratch[i * W];
#pragma unroll
        for (int q = 1; q < W; ++q) r = fmaxf(r, scratch[i * W + q]);
        const float base = r == -INFINITY ? 0.f : r;
        const float ws = wave_sum(s[i] * __expf(m[i] - base));
        if (lane == 0) scratch[(M + i) * W + wid] = ws;
        m[i] = r;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < M; ++i) {
        float r = 0.f;
#pragma unroll
        for (int q = 0; q < W; ++q) r += scratch[(M + i) * W + q];
        s[i] = r;
    }
}

}  // namespace capmi
