// Stochastic beam search (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them"): one selection step and
// the final backtrack (gfx950).  Keeping, at every step, the bd children with the largest PERTURBED log-probability -- Gumbel
// noise on phi, each parent's children conditioned on having the parent's perturbed value as their maximum -- returns bd distinct
// sequences distributed as a sample without replacement from the model.  See include/capmi.h for the arithmetic.
//
// A step is two launches (the chunk-list scheme of search_common.h):
//   sbs_row_kernel    one workgroup per (search row, chunk of 1024 tokens): s = phi + logp + Gumbel for the chunk -- ONE Philox
//                     quad or one 16-byte load of injected noise per thread, the four values never leave its registers -- and
//                     the chunk's bd largest s, in order, to scratch.  B*cur*ceil(V1/1024) workgroups: 500 .. 5000 at the
//                     eval shapes (B 10..50, bd 5..10, V1 9488), where one workgroup per image (beam.hip) would use 10..50 CUs.
//   sbs_merge_kernel  one workgroup per image over the small candidate lists: every row's bd largest s out of its chunks' (the
//                     conditional transform is monotone in s within a row, so nothing else can be kept), the transform on those
//                     cur*bd candidates, and the bd largest results.
// Both rank by counting (value descending, then the lower token / flat index), so the result does not depend on any arrival
// order: plain stores, no float atomics, bit-identical from run to run.
#include "search_common.h"

using namespace capmi;

namespace {

constexpr int MERGE_T = 256;               // >= BD_MAX * BD_MAX: one thread per transformed candidate
constexpr int MERGE_LDS = 48 * 1024;       // the chunk lists of as many rows as fit are staged at once
constexpr uint64_t SBS_STREAM = 0x73627300ull;      // "sbs": the high counter word, apart from the sampling kernels' streams

// log(1 - exp(d)) for d <= 0 without the cancellation of log1p(-exp(d)) near d = 0
__device__ __forceinline__ float log1mexp(float d) { return d > -0.6931472f ? logf(-expm1f(d)) : log1pf(-expf(d)); }

__global__ __launch_bounds__(ROW_T) void sbs_row_kernel(const float *__restrict__ logp, const float *__restrict__ phi,
                                                        const uint8_t *__restrict__ alive, const float *__restrict__ gumbel,
                                                        uint64_t seed, uint32_t offset, const uint64_t *__restrict__ epoch,
                                                        int bd, int V1, int C, int vec, float *__restrict__ cand_s,
                                                        int *__restrict__ cand_tok) {
    __shared__ float s_v[ROW_T / 64];
    __shared__ int s_i[ROW_T / 64];
    const int row = blockIdx.x, chunk = blockIdx.y;
    if (!alive[row]) return;                               // an ended hypothesis has one candidate, made by the merge
    const int q = chunk * ROW_T + threadIdx.x, v0 = 4 * q;
    const float base = phi[row];
    const float *lp = logp + (size_t)row * V1;
    float x[4], gn[4];
    if (vec && v0 + 3 < V1) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(lp + v0);
        x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = v0 + k < V1 ? lp[v0 + k] : -INFINITY;
    }
    if (gumbel) {
        const float *g = gumbel + (size_t)row * V1;
        if (vec && v0 + 3 < V1) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(g + v0);
            gn[0] = t[0]; gn[1] = t[1]; gn[2] = t[2]; gn[3] = t[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) gn[k] = v0 + k < V1 ? g[v0 + k] : 0.f;
        }
    } else {
        const Philox rng(epoch_seed(seed, epoch));
        uint32_t o[4];
        rng.gen(((uint64_t)offset << 32) | (uint32_t)row, (SBS_STREAM << 32) | (uint32_t)q, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) gn[k] = gumbel_u32(o[k]);
    }
    // the thread's four candidates; a -inf log-prob (a decoding constraint, or a column past V1) stays -inf and keeps its token
    Cand c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = Cand{x[k] == -INFINITY ? -INFINITY : (base + x[k]) + gn[k], v0 + k};
    const size_t o0 = ((size_t)row * C + chunk) * bd;
    select_rounds(c, bd, s_v, s_i, cand_s + o0, cand_tok + o0);
}

__global__ __launch_bounds__(MERGE_T) void sbs_merge_kernel(const float *__restrict__ logp, const float *__restrict__ phi,
                                                            const float *__restrict__ g, const uint8_t *__restrict__ alive,
                                                            const float *__restrict__ cand_s, const int *__restrict__ cand_tok,
                                                            int cur, int bd, int V1, int C, int rows_fit, int step0,
                                                            int force_end, int32_t *__restrict__ parent,
                                                            int64_t *__restrict__ token, float *__restrict__ phi_out,
                                                            float *__restrict__ g_out, uint8_t *__restrict__ alive_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float r_s[BD_MAX * BD_MAX];                 // every row's bd largest s, in order
    __shared__ int r_tok[BD_MAX * BD_MAX];
    __shared__ float t_g[BD_MAX * BD_MAX];                 // the transformed candidates
    __shared__ float t_ph[BD_MAX * BD_MAX];
    __shared__ int t_flat[BD_MAX * BD_MAX];                // row * V1 + token < 2^23: C * bd * 8 <= MERGE_LDS bounds cur * V1
    __shared__ int s_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int per_row = C * bd, n = cur * bd;
    float *l_s = reinterpret_cast<float *>(smem);
    int *l_tok = reinterpret_cast<int *>(smem) + (size_t)rows_fit * per_row;
    if (tid < n) {
        r_s[tid] = -INFINITY;
        r_tok[tid] = 0;
    }
    if (tid == 0) s_n = 0;
    // phase A: per row, the bd largest of its C chunk lists (rows_fit rows at a time in LDS)
    for (int j0 = 0; j0 < cur; j0 += rows_fit) {
        const int nr = min(rows_fit, cur - j0), cnt = nr * per_row;
        const size_t src = ((size_t)b * cur + j0) * per_row;
        __syncthreads();
        for (int e = tid; e < cnt; e += MERGE_T) {
            const bool live = alive[(size_t)b * cur + j0 + e / per_row] != 0;      // an ended row's lists were never written
            l_s[e] = live ? cand_s[src + e] : -INFINITY;
            l_tok[e] = live ? cand_tok[src + e] : NO_CAND;
        }
        __syncthreads();
        best_of_lists<MERGE_T>(l_s, l_tok, nr, per_row, bd, r_s + j0 * bd, r_tok + j0 * bd, 0);
    }
    __syncthreads();
    // phase B: the conditional transform on the cur * bd survivors
    if (tid < n) {
        const int j = tid / bd, r = tid - j * bd;
        const size_t row = (size_t)b * cur + j;
        const float pj = phi[row], gj = g[row];
        float gt, ph;
        int tok = 0;
        bool ok;
        if (!alive[row]) {                                 // carried on unchanged: token 0, g bit for bit
            ok = r == 0;
            gt = gj;
            ph = pj;
        } else {
            const float s = r_s[tid], Z = r_s[j * bd];
            ok = s != -INFINITY;
            tok = r_tok[tid];
            ph = ok ? pj + logp[row * V1 + tok] : -INFINITY;
            if (step0 || !ok) {
                gt = s;                                    // no conditioning at the root
            } else if (r == 0) {
                gt = gj;                                   // the arg-max inherits the parent's value exactly
            } else {
                const float u = gj - s + log1mexp(s - Z);
                gt = gj - fmaxf(0.f, u) - log1pf(expf(-fabsf(u)));
            }
        }
        t_g[tid] = ok ? gt : -INFINITY;                    // what is no candidate: {-inf, NO_CAND}
        t_flat[tid] = ok ? j * V1 + tok : NO_CAND;
        t_ph[tid] = ph;
        r_tok[tid] = tok;                                  // read by this thread alone from here on
    }
    __syncthreads();
    // phase C: the bd largest, ties to the lower flat index
    best_of_candidates<MERGE_T>(
        t_g, t_flat, n, bd, &s_n,
        [&](int rank, int e) {                             // e == tid: one candidate per thread
            const size_t o = (size_t)b * bd + rank;
            const int tok = r_tok[e];
            const bool was = alive[(size_t)b * cur + e / bd] != 0;
            parent[o] = e / bd;
            token[o] = tok;
            phi_out[o] = t_ph[e];
            g_out[o] = t_g[e];
            alive_out[o] = (was && tok != 0 && !force_end) ? 1 : 0;
        },
        [&](int slot) {                                    // fewer than bd finite candidates (not visible from the arguments)
            const size_t o = (size_t)b * bd + slot;
            parent[o] = 0;
            token[o] = 0;
            phi_out[o] = -INFINITY;
            g_out[o] = -INFINITY;
            alive_out[o] = 0;
        });
}

__global__ void sbs_backtrack_kernel(const int32_t *__restrict__ parent, const int64_t *__restrict__ token,
                                     const uint8_t *__restrict__ alive, int B, int bd, int L, int64_t *__restrict__ seq,
                                     int32_t *__restrict__ length, int32_t *__restrict__ lineage) {
    const int rows = B * bd, row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int b = row / bd;
    // the whole length: the earliest step of the path that is not alive is its end
    length[row] = backtrack_path(parent, token, alive, B, bd, L, b, L - 1, row - b * bd, seq + (size_t)row * L, lineage + row, rows);
}

}  // namespace

extern "C" {

int64_t capmi_sbs_scratch_bytes(int B, int cur, int bd, int V1) { return chunk_lists_bytes(B, cur, bd, V1, 0); }

int capmi_sbs_select(const float *logp, const float *phi, const float *g, const uint8_t *alive, const float *gumbel,
                     uint64_t seed, uint32_t offset, int B, int cur, int bd, int V1, int step0, int force_end, void *scratch,
                     int64_t scratch_bytes, int32_t *parent, int64_t *token, float *phi_out, float *g_out, uint8_t *alive_out,
                     void *stream) {
    if (!logp || !phi || !g || !alive || !scratch || !parent || !token || !phi_out || !g_out || !alive_out) return CAPMI_EINVAL;
    if (B <= 0 || cur <= 0 || cur > bd || bd > BD_MAX || V1 <= 0 || (long long)cur * V1 < bd || (step0 && cur != 1))
        return CAPMI_EINVAL;
    const int C = chunks_of(V1, 0);
    const long long per_row = (long long)C * bd;
    ChunkLists cand;
    if ((long long)B * cur > 0x7fffffffLL || C > 65535 || per_row * 8 > MERGE_LDS) return CAPMI_EINVAL;
    if (!chunk_lists(scratch, scratch_bytes, B, cur, bd, V1, 0, &cand)) return CAPMI_EINVAL;
    const int vec = (V1 % 4 == 0 && aligned16(logp, gumbel)) ? 1 : 0;
    hipLaunchKernelGGL(sbs_row_kernel, dim3(B * cur, C), dim3(ROW_T), 0, (hipStream_t)stream, logp, phi, alive, gumbel, seed,
                       offset, gumbel ? nullptr : rng_epoch(), bd, V1, C, vec, cand.s, cand.tok);
    CAPMI_CHECK_LAUNCH();
    int rows_fit = (int)(MERGE_LDS / (per_row * 8));
    if (rows_fit > cur) rows_fit = cur;
    hipLaunchKernelGGL(sbs_merge_kernel, dim3(B), dim3(MERGE_T), (size_t)rows_fit * per_row * 8, (hipStream_t)stream, logp, phi,
                       g, alive, cand.s, cand.tok, cur, bd, V1, C, rows_fit, step0, force_end, parent, token, phi_out, g_out,
                       alive_out);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_sbs_backtrack(const int32_t *parent, const int64_t *token, const uint8_t *alive, int B, int bd, int L, int64_t *seq,
                        int32_t *length, int32_t *lineage, void *stream) {
    if (!parent || !token || !alive || !seq || !length || !lineage) return CAPMI_EINVAL;
    if (B <= 0 || bd <= 0 || bd > BD_MAX || L <= 0) return CAPMI_EINVAL;
    hipLaunchKernelGGL(sbs_backtrack_kernel, dim3(((size_t)B * bd + 255) / 256), dim3(256), 0, (hipStream_t)stream, parent, token,
                       alive, B, bd, L, seq, length, lineage);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
