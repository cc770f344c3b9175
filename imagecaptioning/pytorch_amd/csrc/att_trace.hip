// Per-word region attention of a decoded caption (return_attention): the weights the attention LSTM families already keep on the
// device, brought into one caption-major array, and what a caller reads off it per word.
//
//   capmi_att_trace_rollout   alpha [T, N, K] of a rollout (step-major, clipped K) + seq [N, L]  ->  att [N, L, Kout]
//   capmi_att_trace_beam      alpha_rows [L, rows_src, K] by search row + lineage / length of capmi_beam_finalize -> att [rows, L, Kout]
//   capmi_att_ground          att [N, L, Kw] -> top / top_w / entropy (/ the attention-weighted box) per (row, step)
//
// All three are memory bound and tiny: one wave per (caption row, step), four waves per workgroup, every reduction over the
// region axis inside the wave (the fixed butterflies of capmi_common.h: deterministic), no atomics, no host sync, one launch each.
// A trace row is COPIED, never recomputed, so the output holds the bits the decoder used.  Kept steps are those where
// losses._shifted_mask is 1 (step 0, then every step whose previous token is not 0: the EOS step is kept); every other step and
// every column behind the clipped K is written as 0 -- written, so the output needs no memset and stale or non-finite values in
// the source behind a caption's end (an early exit leaves steps unwritten) never reach it.
// A row of Kout floats is 16-byte aligned only when Kout % 4 == 0: that case stores float4, every other one dwords.
#include "host_common.h"

using namespace capmi;

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / CAPMI_WAVE;

struct TraceArgs {
    const float *alpha;         // rollout: [T, N, K]; beam: [L, rows_src, K]
    const float *beta;          // rollout only, optional [T, N]: a leading column of its own
    const int64_t *seq;         // rollout: [N, L]
    const int32_t *lineage;     // beam: [L, N] search row per (step, output row), < 0 behind the end
    const int32_t *length;      // beam: [N]
    float *att;                 // [N, L, Kout]
    int T, N, L, K, Kout, rows_src;
};

__global__ __launch_bounds__(THREADS) void att_trace_kernel(TraceArgs a) {
    const int lane = threadIdx.x & (CAPMI_WAVE - 1);
    const size_t item = (size_t)blockIdx.x * WAVES + (threadIdx.x / CAPMI_WAVE);         // wave-uniform
    if (item >= (size_t)a.N * a.L) return;
    const int n = (int)(item / a.L), l = (int)(item - (size_t)n * a.L);
    const float *src = nullptr;
    float b0 = 0.f;
    if (a.lineage) {
        const int r = l < a.length[n] ? a.lineage[(size_t)l * a.N + n] : -1;
        if (r >= 0 && r < a.rows_src)
            src = a.alpha + ((size_t)l * a.rows_src + r) * a.K;
    } else if (l < a.T && (l == 0 || a.seq[(size_t)n * a.L + l - 1] > 0)) {
        src = a.alpha + ((size_t)l * a.N + n) * a.K;
        if (a.beta) b0 = a.beta[(size_t)l * a.N + n];
    }
    const int off = a.beta ? 1 : 0;
    auto val = [&](int c) -> float {
        if (!src) return 0.f;
        if (c < off) return b0;
        const int k = c - off;
        return k < a.K ? src[k] : 0.f;
    };
    float *o = a.att + item * a.Kout;
    if ((a.Kout & 3) == 0 && (reinterpret_cast<uintptr_t>(a.att) & 15) == 0) {
        f32x4 *o4 = reinterpret_cast<f32x4 *>(o);
        for (int q = lane; q < a.Kout / 4; q += CAPMI_WAVE) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = val(4 * q + e);
            o4[q] = v;
        }
    } else {
        for (int c = lane; c < a.Kout; c += CAPMI_WAVE) o[c] = val(c);
    }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// boxes [B, Kb, 4] are the boxes of att's columns col0 .. col0 + Kb - 1 (col0 = 1: the AdaAtt sentinel column has no box)
__global__ __launch_bounds__(THREADS) void att_ground_kernel(const float *__restrict__ att, const f32x4 *__restrict__ boxes,
                                                            int N, int L, int Kw, int n_per_image, int col0, int Kb,
                                                            int32_t *__restrict__ top, float *__restrict__ top_w,
                                                            float *__restrict__ entropy, f32x4 *__restrict__ box) {
    const int lane = threadIdx.x & (CAPMI_WAVE - 1);
    const size_t item = (size_t)blockIdx.x * WAVES + (threadIdx.x / CAPMI_WAVE);         // wave-uniform
    if (item >= (size_t)N * L) return;
    const float *x = att + item * Kw;
    const f32x4 *bx = boxes ? boxes + (size_t)((item / L) / n_per_image) * Kb : nullptr;
    float best = -1.f, ent = 0.f;
    int best_k = 0x7fffffff;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < Kw; k += CAPMI_WAVE) {
        const float v = x[k];
        if (v > best) { best = v; best_k = k; }             // ascending k: the first of equal values stays
        if (v > 0.f) ent -= v * logf(v);                    // 0 * ln 0 = 0
        if (bx && k >= col0 && k - col0 < Kb) {
            const f32x4 b = bx[k - col0];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += v * b[e];
        }
    }
    const float m = wave_max(best);
    const int k_top = wave_min_i(best == m ? best_k : 0x7fffffff);                       // ties: the lowest index
    ent = wave_sum(ent);
    if (bx) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = wave_sum(acc[e]);
    }
    if (lane == 0) {
        const bool kept = m > 0.f;                          // a zeroed step holds no positive weight
        top[item] = kept ? k_top : -1;
        top_w[item] = kept ? m : 0.f;
        entropy[item] = kept ? ent : 0.f;
        if (box) box[item] = acc;
    }
}

inline bool off4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

int launch_trace(const TraceArgs &a, void *stream) {
    const size_t items = (size_t)a.N * a.L;
    hipLaunchKernelGGL(att_trace_kernel, dim3((unsigned)((items + WAVES - 1) / WAVES)), dim3(THREADS), 0, (hipStream_t)stream, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int capmi_att_trace_rollout(const float *alpha, const float *beta, const int64_t *seq, int T, int N, int L, int K, int Kout,
                            float *att, void *stream) {
    if (!alpha || !seq || !att || T <= 0 || N <= 0 || L <= 0 || K <= 0 || T > L) return CAPMI_EINVAL;
    if (K + (beta ? 1 : 0) > Kout || (long long)N * L > 0x7fffffffLL) return CAPMI_EINVAL;
    if (off4(alpha) || off4(beta) || off4(att) || (reinterpret_cast<uintptr_t>(seq) & 7)) return CAPMI_EINVAL;
    const TraceArgs a{alpha, beta, seq, nullptr, nullptr, att, T, N, L, K, Kout, N};
    return launch_trace(a, stream);
}

int capmi_att_trace_beam(const float *alpha_rows, const int32_t *lineage, const int32_t *length, int L, int rows_src, int rows, int K,
                         int Kout, float *att, void *stream) {
    if (!alpha_rows || !lineage || !length || !att || L <= 0 || rows_src <= 0 || rows <= 0 || K <= 0) return CAPMI_EINVAL;
    if (K > Kout || (long long)rows * L > 0x7fffffffLL) return CAPMI_EINVAL;
    if (off4(alpha_rows) || off4(att) || off4(lineage) || off4(length)) return CAPMI_EINVAL;
    const TraceArgs a{alpha_rows, nullptr, nullptr, lineage, length, att, L, rows, L, K, Kout, rows_src};
    return launch_trace(a, stream);
}

int capmi_att_ground(const float *att, int N, int L, int Kw, const float *boxes, int B, int n, int col0, int Kb, int32_t *top,
                     float *top_w, float *entropy, float *box, void *stream) {
    if (!att || !top || !top_w || !entropy || N <= 0 || L <= 0 || Kw <= 0 || (long long)N * L > 0x7fffffffLL) return CAPMI_EINVAL;
    if (off4(att) || off4(top) || off4(top_w) || off4(entropy)) return CAPMI_EINVAL;
    if ((boxes != nullptr) != (box != nullptr)) return CAPMI_EINVAL;
    if (boxes) {
        // every row's image r / n must be one of the B box sets, and the boxed columns must exist
        if (B <= 0 || n <= 0 || (long long)B * n < N || col0 < 0 || Kb <= 0 || col0 + Kb > Kw || !aligned16(boxes, box))
            return CAPMI_EINVAL;
    }
    const size_t items = (size_t)N * L;
    hipLaunchKernelGGL(att_ground_kernel, dim3((unsigned)((items + WAVES - 1) / WAVES)), dim3(THREADS), 0, (hipStream_t)stream, att,
                       reinterpret_cast<const f32x4 *>(boxes), N, L, Kw, boxes ? n : 1, col0, Kb, top, top_w, entropy,
                       reinterpret_cast<f32x4 *>(box));
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
