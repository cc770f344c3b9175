// Scoring given captions (gfx950): log p(token | image, prefix) of ONE given token per decoder row, and the ranks of a
// caption-by-image score matrix (score.py, mode='score', tools/eval.py --self_retrieval / --score_json).  See include/capmi.h for
// the arithmetic.
//
// score_step_kernel    a row of logits is read ONCE: every thread keeps a running (max, sum of exp) pair over its share of the row
//                      -- an online logsumexp -- and the pairs are merged by a wave / block max followed by a wave / block sum of
//                      the rescaled sums, both in the fixed order of capmi_common.h: no atomics, the same bits from run to run.
//                      Nothing of the row's size is written; the step is bound by the rows * V1 * 4 bytes it reads.
//                      The row is cut on its OWN alignment (row_sweep.h), so ld and V1 need not be multiples of 4.
//                      Launch shape by V1: up to WAVE_V1 columns one WAVE per row (four rows per 256-thread workgroup, no LDS, no
//                      barrier: a 4 KB row is 4 loads per lane); above, one 256-thread WORKGROUP per row (a 37 KB row of the 9488
//                      word vocabulary is 9-10 16-byte loads per thread, all in flight at once; 8000 rows are 8000 workgroups).
// retrieval_rank_kernel  one workgroup per caption over its row of I scores: integer counts (order-free) and the same online
//                      logsumexp for the posterior.
#include "host_common.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int SC_T = 256;
constexpr int WAVE_V1 = 1024;              // rows of up to this many columns: a wave each

// running logsumexp pair; m = -inf, s = 0 is the empty one
struct LSE {
    float m, s;
};
__device__ __forceinline__ void lse_add(LSE &a, float y) {
    const float mn = fmaxf(a.m, y);
    if (mn > -INFINITY) {                  // (a NaN or all -inf so far: nothing to add)
        a.s = a.s * __expf(a.m - mn) + __expf(y - mn);
        a.m = mn;
    }
}
__device__ __forceinline__ void lse_add4(LSE &a, float y0, float y1, float y2, float y3) {
    const float mn = fmaxf(fmaxf(a.m, fmaxf(y0, y1)), fmaxf(y2, y3));
    if (mn > -INFINITY) {
        a.s = a.s * __expf(a.m - mn) + ((__expf(y0 - mn) + __expf(y1 - mn)) + (__expf(y2 - mn) + __expf(y3 - mn)));
        a.m = mn;
    }
}

// this thread's share of x[0, n) * scale; tid of nthr threads (a wave or a workgroup).  The cut is row_sweep.h's; the order is this
// file's own -- head, body, tail, the head and the tail one guarded element each (at most 3 columns) -- and stays: the payload is
// not associative in float, so row_sweep.h's sweep (body, head, tail) would give other bits.
__device__ __forceinline__ LSE lse_scan(const float *__restrict__ x, int n, float scale, int tid, int nthr) {
    LSE a{-INFINITY, 0.f};
    const RowSplit sp = row_split(x, n, true);
    if (tid < sp.head) lse_add(a, x[tid] * scale);
    for (int i = tid; i < sp.nv; i += nthr) {
        const f32x4 v = ld4(x + sp.head + 4 * i);
        lse_add4(a, v.x * scale, v.y * scale, v.z * scale, v.w * scale);
    }
    if (tid < n - sp.tail) lse_add(a, x[sp.tail + tid] * scale);
    return a;
}

__device__ __forceinline__ float rescaled(LSE a, float m) { return a.m > -INFINITY ? a.s * __expf(a.m - m) : 0.f; }

template <bool WAVE>
__global__ __launch_bounds__(SC_T) void score_step_kernel(const float *__restrict__ logits, int64_t ld, int rows, int V1,
                                                          const int64_t *__restrict__ tok, uint8_t *__restrict__ live,
                                                          float *__restrict__ acc, int32_t *__restrict__ cnt,
                                                          float *__restrict__ tok_logp, float inv_t, int unk_col) {
    __shared__ float s_f[32];
    const int lane = threadIdx.x & 63;
    const int row = WAVE ? (int)blockIdx.x * (SC_T / 64) + (threadIdx.x >> 6) : (int)blockIdx.x;
    if (row >= rows || !live[row]) return;            // uniform over the wave (WAVE) / the workgroup: no barrier is left waiting
    const float *x = logits + (size_t)row * ld;
    const LSE a = lse_scan(x, V1, inv_t, WAVE ? lane : (int)threadIdx.x, WAVE ? 64 : SC_T);
    float m, s;
    if constexpr (WAVE) {
        m = wave_max(a.m);
        s = wave_sum(rescaled(a, m));
    } else {
        m = block_max(a.m, s_f);
        s = block_sum(rescaled(a, m), s_f);
    }
    if ((WAVE ? lane : (int)threadIdx.x) != 0) return;
    const int64_t v = tok[row];
    float lp = __builtin_nanf("");                    // a token outside [0, V1) (the driver refuses it on the host) reads nothing
    if (v >= 0 && v < V1) {
        lp = x[v] * inv_t - (m + logf(s));
        if (v == unk_col) lp -= 1000.f;               // = capmi_beam_logsoftmax: normalised over every column, then pushed down
    }
    acc[row] += lp;
    cnt[row] += 1;
    if (tok_logp) tok_logp[row] = lp;
    if (v == 0) live[row] = 0;                        // the end token is scored, then the row is dead
}

__global__ __launch_bounds__(SC_T) void retrieval_rank_kernel(const float *__restrict__ S, int64_t ld, int I,
                                                              const int32_t *__restrict__ target, int32_t *__restrict__ rank,
                                                              float *__restrict__ log_post) {
    __shared__ float s_f[32];
    __shared__ int s_n;
    const int c = blockIdx.x, t = target[c];
    if (t < 0 || t >= I) {                            // refused on the host (ops.retrieval_rank); nothing is read
        if (threadIdx.x == 0) {
            rank[c] = 0;
            if (log_post) log_post[c] = __builtin_nanf("");
        }
        return;
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const float *x = S + (size_t)c * ld;
    const float st = x[t];
    int n = 0;
    for (int i = threadIdx.x; i < I; i += SC_T) {
        const float v = x[i];
        n += (v > st) || (v == st && i < t);
    }
    if (n) atomicAdd(&s_n, n);                        // LDS, integers: the sum does not depend on the order
    if (log_post) {                                   // uniform
        const LSE a = lse_scan(x, I, 1.f, threadIdx.x, SC_T);
        const float m = block_max(a.m, s_f);
        const float s = block_sum(rescaled(a, m), s_f);
        if (threadIdx.x == 0) log_post[c] = st - (m + logf(s));
    }
    __syncthreads();
    if (threadIdx.x == 0) rank[c] = 1 + s_n;
}

}  // namespace

extern "C" {

int capmi_score_step(const float *logits, int64_t ld, int rows, int V1, const int64_t *tok, uint8_t *live, float *acc, int32_t *cnt,
                     float *tok_logp, float inv_temperature, int unk_col, void *stream) {
    if (!logits || !tok || !live || !acc || !cnt) return CAPMI_EINVAL;
    if (rows <= 0 || V1 <= 0 || ld < V1 || !(inv_temperature > 0.f) || !(inv_temperature < INFINITY)) return CAPMI_EINVAL;
    if (V1 <= WAVE_V1)
        hipLaunchKernelGGL(score_step_kernel<true>, dim3((rows + SC_T / 64 - 1) / (SC_T / 64)), dim3(SC_T), 0, (hipStream_t)stream,
                           logits, ld, rows, V1, tok, live, acc, cnt, tok_logp, inv_temperature, unk_col);
    else
        hipLaunchKernelGGL(score_step_kernel<false>, dim3(rows), dim3(SC_T), 0, (hipStream_t)stream, logits, ld, rows, V1, tok, live,
                           acc, cnt, tok_logp, inv_temperature, unk_col);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_retrieval_rank(const float *S, int64_t ld, int C, int I, const int32_t *target, int32_t *rank, float *log_post,
                         void *stream) {
    if (!S || !target || !rank) return CAPMI_EINVAL;
    if (C <= 0 || I <= 0 || ld < I) return CAPMI_EINVAL;
    hipLaunchKernelGGL(retrieval_rank_kernel, dim3(C), dim3(SC_T), 0, (hipStream_t)stream, S, ld, I, target, rank, log_post);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
