// Contrastive search decoding (gfx950; Su et al. 2022, "A Contrastive Framework for Neural Text Generation").  See include/capmi.h
// (capmi_contrastive_topk, capmi_contrastive_select) for the contract.  Per generated token the driver (decode.contrastive_steps)
// launches the top-k kernel on the N constrained log-prob rows, steps the decoder on the N * k candidate rows and launches the select
// kernel, which scores the candidates against the row's hidden-state history and writes everything the next step needs.
//
//   topk    one workgroup of 16 wave64s per row; k rounds of a block-wide arg-max over the 64-bit key (orderable value bits, ~id), each
//           round taking the largest key below the previous winner: value descending, ties to the lower id, -inf entries like any
//           other value.  The row (38 KB at V1 = 9488) is re-read from cache per round; the last pass stores logp * unfinished.
//   select  one workgroup of 4 wave64s per row; wave w takes the candidates w, w + 4, ...: |g|^2 (in double), then the dots with the history rows
//           four at a time (g is loaded once per four rows), fp32, 16-byte loads in the VEC arm.  Nothing of width R is staged in LDS:
//           the rows stream, R has no upper bound.  Thread 0 takes the arg-max and writes the index outputs; all threads copy the
//           winner's row behind the history.
#include "host_common.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int TK_T = 1024;
constexpr int TK_W = TK_T / 64;
constexpr int CS_T = 256;
constexpr int CS_W = CS_T / 64;
constexpr int CS_SB = 4;               // history rows per pass over a candidate row

// a float as an unsigned that orders like the float (-inf lowest, -0 below +0: callers add +0.f first)
__device__ __forceinline__ uint32_t ord_f(float x) {
    const uint32_t u = f2u(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f(uint32_t o) { return u2f((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = __shfl_xor(v, o, 64);
        v = y > v ? y : v;
    }
    return v;
}

__global__ __launch_bounds__(TK_T) void contrastive_topk_kernel(const float *__restrict__ logp, int ld, int V1, int k,
                                                               const uint8_t *__restrict__ unfinished, int64_t *__restrict__ tok,
                                                               float *__restrict__ tok_logp, float *__restrict__ store,
                                                               int64_t store_ld) {
    __shared__ uint64_t s_k[TK_W];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *row = logp + (size_t)r * ld;
    uint64_t prev = ~0ull;
    for (int round = 0; round < k; ++round) {
        uint64_t best = 0;                       // every real key is above 0 (ord_f(-inf) = 0x007fffff)
        for (int v = tid; v < V1; v += TK_T) {
            const uint64_t key = ((uint64_t)ord_f(row[v] + 0.f) << 32) | (uint32_t)(0xffffffffu - (uint32_t)v);
            if (key < prev && key > best) best = key;
        }
        best = wave_max_u64(best);
        __syncthreads();                         // s_k of the round before has been read
        if ((tid & 63) == 0) s_k[tid >> 6] = best;
        __syncthreads();
        best = s_k[0];
#pragma unroll
        for (int w = 1; w < TK_W; ++w) best = s_k[w] > best ? s_k[w] : best;
        prev = best;
        if (tid == 0) {
            tok[(size_t)r * k + round] = (int64_t)(0xffffffffu - (uint32_t)best);
            tok_logp[(size_t)r * k + round] = unord_f((uint32_t)(best >> 32));
        }
    }
    if (store) {
        float *sr = store + (size_t)r * store_ld;
        const bool unf = unfinished ? unfinished[r] != 0 : true;
        for (int v = tid; v < V1; v += TK_T) sr[v] = unf ? row[v] : row[v] * 0.f;
    }
}

struct SelectArgs {
    const int64_t *cand_tok;
    const float *cand_logp, *cand_h;
    float *hist, *hist_inv;
    int32_t *choice, *parent, *fan;
    int64_t *seq, *it;
    uint8_t *unfinished;
    int k, R, ld, S_max, hist_len, t, seq_ld;
    float alpha;
};

// dot products of g [R] with n <= CS_SB history rows h, h + R, ..., summed over the wave
template <bool VEC>
__device__ __forceinline__ void dots(const float *__restrict__ g, const float *__restrict__ h, int R, int n, int lane,
                                     float (&acc)[CS_SB]) {
#pragma unroll
    for (int u = 0; u < CS_SB; ++u) acc[u] = 0.f;
    if (VEC) {
        for (int c = 4 * lane; c < R; c += 4 * 64) {
            const f32x4 a = ld4(g + c);
#pragma unroll
            for (int u = 0; u < CS_SB; ++u)
                if (u < n) {
                    const f32x4 b = ld4(h + (size_t)u * R + c);
                    acc[u] += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
                }
        }
    } else {
        for (int c = lane; c < R; c += 64) {
            const float a = g[c];
#pragma unroll
            for (int u = 0; u < CS_SB; ++u)
                if (u < n) acc[u] += a * h[(size_t)u * R + c];
        }
    }
#pragma unroll
    for (int u = 0; u < CS_SB; ++u) acc[u] = wave_sum(acc[u]);
}

template <bool VEC>
__global__ __launch_bounds__(CS_T) void contrastive_select_kernel(const SelectArgs a) {
    __shared__ float s_score[CAPMI_CONTRASTIVE_KMAX], s_inv[CAPMI_CONTRASTIVE_KMAX];
    __shared__ int s_choice;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int k = a.k, R = a.R, len = a.hist_len;
    const float *hrow = a.hist + (size_t)i * a.S_max * R;
    const float *hinv = a.hist_inv + (size_t)i * a.S_max;
    for (int j = wid; j < k; j += CS_W) {               // uniform over the wave
        const float *g = a.cand_h + ((size_t)i * k + j) * a.ld;
        // |g|^2 in double: the inverse norm is stored beside the history row and is good to an ulp of float at any R
        double nn = 0.0;
        if (VEC) {
            for (int c = 4 * lane; c < R; c += 4 * 64) {
                const f32x4 x = ld4(g + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) nn += (double)x[e] * (double)x[e];
            }
        } else {
            for (int c = lane; c < R; c += 64) nn += (double)g[c] * (double)g[c];
        }
        nn = wave_sum_d(nn);
        const float inv_g = (float)(1.0 / sqrt(nn));     // a zero row: inf, and every cosine below is 0 * 1e8 = 0
        float worst = len > 0 ? -INFINITY : 0.f;         // max over s of cos(g, h_s); an empty history penalises nothing
        for (int s0 = 0; s0 < len; s0 += CS_SB) {
            const int n = len - s0 < CS_SB ? len - s0 : CS_SB;
            float acc[CS_SB];
            dots<VEC>(g, hrow + (size_t)s0 * R, R, n, lane, acc);
#pragma unroll
            for (int u = 0; u < CS_SB; ++u)
                if (u < n) worst = fmaxf(worst, acc[u] * fminf(inv_g * hinv[s0 + u], 1e8f));   // a.b / max(|a| |b|, 1e-8)
        }
        if (lane == 0) {
            const float lp = a.cand_logp ? a.cand_logp[(size_t)i * k + j] : -INFINITY;
            s_score[j] = lp == -INFINITY ? -INFINITY : (1.f - a.alpha) * expf(lp) - a.alpha * worst;
            s_inv[j] = inv_g;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        float best = s_score[0];
        for (int j = 1; j < k; ++j)
            if (s_score[j] > best) best = s_score[j], c = j;      // lowest j on ties; all -inf: candidate 0
        s_choice = c;
        if (a.choice) a.choice[i] = c;
        if (a.parent) a.parent[i] = i * k + c;
        if (a.fan)
            for (int j = 0; j < k; ++j) a.fan[(size_t)i * k + j] = c;
        if (a.cand_tok) {
            const bool unf = a.unfinished ? a.unfinished[i] != 0 : true;
            const int64_t tok = unf ? a.cand_tok[(size_t)i * k + c] : 0;
            if (a.seq) a.seq[(size_t)i * a.seq_ld + a.t] = tok;
            if (a.it) a.it[i] = tok;
            if (a.unfinished) a.unfinished[i] = unf && tok != 0 ? 1 : 0;
        }
        a.hist_inv[(size_t)i * a.S_max + len] = s_inv[c];
    }
    __syncthreads();
    const float *g = a.cand_h + ((size_t)i * k + s_choice) * a.ld;
    float *dst = a.hist + ((size_t)i * a.S_max + len) * R;
    if (VEC) {
        for (int c = 4 * tid; c < R; c += 4 * CS_T) st4(dst + c, ld4(g + c));
    } else {
        for (int c = tid; c < R; c += CS_T) dst[c] = g[c];
    }
}

}  // namespace

extern "C" int capmi_contrastive_topk(const float *logp, int ld, int N, int V1, int k, const uint8_t *unfinished, int64_t *tok,
                                      float *tok_logp, float *store, int64_t store_ld, void *stream) {
    if (!logp || !tok || !tok_logp || N < 0 || V1 <= 0 || ld < V1 || k < 1 || k > CAPMI_CONTRASTIVE_KMAX || k > V1)
        return CAPMI_EINVAL;
    if (!aligned4(logp, tok_logp, store) || (reinterpret_cast<uintptr_t>(tok) & 7)) return CAPMI_EINVAL;
    if (store) {
        if (store_ld < V1) return CAPMI_EINVAL;
        if (N > 0 && overlaps(store, ((size_t)(N - 1) * (size_t)store_ld + V1) * sizeof(float), logp, span(N, ld, V1))) return CAPMI_EINVAL;
    }
    if (N == 0) return 0;
    hipLaunchKernelGGL(contrastive_topk_kernel, dim3(N), dim3(TK_T), 0, (hipStream_t)stream, logp, ld, V1, k, unfinished, tok,
                       tok_logp, store, store_ld);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_contrastive_select(const int64_t *cand_tok, const float *cand_logp, const float *cand_h, int ld, float *hist,
                                        float *hist_inv, int N, int k, int R, int S_max, int hist_len, int t, int L, float alpha,
                                        int32_t *choice, int32_t *parent, int32_t *fan, int64_t *seq, int seq_ld, int64_t *it,
                                        uint8_t *unfinished, void *stream) {
    if (!cand_h || !hist || !hist_inv || N < 0 || k < 1 || k > CAPMI_CONTRASTIVE_KMAX || R < 1 || ld < R) return CAPMI_EINVAL;
    if (L < 1 || t < 0 || t >= L || S_max < L + 1 || hist_len < 0 || hist_len >= S_max) return CAPMI_EINVAL;
    if (!(alpha >= 0.f && alpha <= 1.f)) return CAPMI_EINVAL;                       // (also NaN)
    if (seq && seq_ld < L) return CAPMI_EINVAL;
    if (!aligned4(cand_logp, cand_h, hist, hist_inv, choice, parent, fan)) return CAPMI_EINVAL;
    if ((reinterpret_cast<uintptr_t>(cand_tok) | reinterpret_cast<uintptr_t>(seq) | reinterpret_cast<uintptr_t>(it)) & 7) return CAPMI_EINVAL;
    if ((int64_t)N * k > INT32_MAX) return CAPMI_EINVAL;
    if (N == 0) return 0;
    if (overlaps(cand_h, span(N * k, ld, R), hist, (size_t)N * S_max * R * sizeof(float))) return CAPMI_EINVAL;
    SelectArgs a{};
    a.cand_tok = cand_tok;
    a.cand_logp = cand_logp;
    a.cand_h = cand_h;
    a.hist = hist;
    a.hist_inv = hist_inv;
    a.choice = choice;
    a.parent = parent;
    a.fan = fan;
    a.seq = seq;
    a.it = it;
    a.unfinished = unfinished;
    a.k = k;
    a.R = R;
    a.ld = ld;
    a.S_max = S_max;
    a.hist_len = hist_len;
    a.t = t;
    a.seq_ld = seq_ld;
    a.alpha = alpha;
    const bool vec = R % 4 == 0 && ld % 4 == 0 && aligned16(cand_h, hist);
    if (vec)
        hipLaunchKernelGGL(contrastive_select_kernel<true>, dim3(N), dim3(CS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(contrastive_select_kernel<false>, dim3(N), dim3(CS_T), 0, (hipStream_t)stream, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
