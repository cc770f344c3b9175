// Constrained beam search (Anderson, Fernando, Johnson and Gould 2017, "Guided Open Vocabulary Image Captioning with Constrained
// Beam Search"): one selection step and the finalisation (gfx950).  A hypothesis's state is the bitmask of the constraints it has
// satisfied; an image keeps one beam of b slots per state (slot = state * b + j), and a token of a constraint's word set moves the
// hypothesis to the state with that bit set.  See include/capmi.h for the arithmetic.
//
// A step is two launches:
//   cbs_row_kernel    one workgroup per (search row, chunk of 1024 floats): the STAYING candidates of the row -- every token that is
//                     in no unsatisfied word set -- and the chunk's b largest scores, in order, to scratch.  The row is read once,
//                     in 16-byte pieces: the chunks are cut on the 16-byte grid of the row's own address, so a row that starts off
//                     the grid (V1 no multiple of 4) has a scalar head in its first chunk and a scalar tail in its last.  The <= 32
//                     listed tokens are knocked out through a 1024-bit map in LDS, not searched for per token.
//   cbs_merge_kernel  one workgroup per (image, target state s'): the b best staying candidates of each row in s' out of its chunk
//                     lists, the MOVING candidates -- enumerated: every valid row of a state s that is a proper subset of s' times
//                     the listed tokens v with s | sat(v) == s' -- and the b best of both, ranked by counting.
// Order everywhere: larger score first, equal scores by the lower flat index row * V1 + token.  Plain stores, no float atomics:
// bit-identical from run to run.
#include "search_common.h"

using namespace capmi;

namespace {

constexpr int MERGE_T = 256;
constexpr int C_MAX = 4, W_MAX = 8, NW = C_MAX * W_MAX;
constexpr int SB_MAX = 64;                 // slots per image
constexpr int STAGE_MAX = 2048;            // chunk-list entries of one row staged in LDS
constexpr int CAND_MAX = 4096;             // S = 1: b * b <= 4096; S > 1 (b <= 32): b * b + 64 * 32 <= 3072
constexpr int FIN_T = 256;
constexpr int FIN_MAX = 4096;              // L * S * b finished candidates of an image

__device__ __forceinline__ int clamp_ncons(int n, int S) {
    n = n < 0 ? 0 : (n > C_MAX ? C_MAX : n);
    while ((1 << n) > S) --n;
    return n;
}

__global__ __launch_bounds__(ROW_T) void cbs_row_kernel(const float *__restrict__ logp, const float *__restrict__ sums,
                                                        const int32_t *__restrict__ words, const int32_t *__restrict__ ncons,
                                                        int cur, int b, int S, int V1, int C, float *__restrict__ cand_s,
                                                        int *__restrict__ cand_tok) {
    __shared__ float s_v[ROW_T / 64];
    __shared__ int s_i[ROW_T / 64];
    __shared__ unsigned s_out[CHUNK / 32];                 // tokens of the chunk that may not stay: bit = position in the chunk
    const int row = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int img = row / cur, slot = row - img * cur;
    const float base = sums[(size_t)img * S * b + slot];
    if (!(base > -INFINITY)) return;                       // an empty slot is never a source (the merge tests the same value)
    const int state = cur == 1 ? 0 : slot / b;
    const float *lp = logp + (size_t)row * V1;
    const int a = (int)((reinterpret_cast<uintptr_t>(lp) >> 2) & 3);       // floats from the 16-byte grid to the row's start
    if (tid < CHUNK / 32) s_out[tid] = 0u;
    __syncthreads();
    if (tid < NW) {
        const int c = tid / W_MAX, v = words[(size_t)img * NW + tid];
        if (c < clamp_ncons(ncons[img], S) && !((state >> c) & 1) && v >= 0 && v < V1) {
            const int p = v + a - chunk * CHUNK;
            if (p >= 0 && p < CHUNK) atomicOr(&s_out[p >> 5], 1u << (p & 31));
        }
    }
    __syncthreads();
    const int p0 = chunk * CHUNK + 4 * tid, v0 = p0 - a;   // lp + v0 is on the 16-byte grid
    float x[4];
    if (v0 >= 0 && v0 + 3 < V1) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(lp + v0);
        x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (v0 + k >= 0 && v0 + k < V1) ? lp[v0 + k] : -INFINITY;
    }
    const unsigned out4 = (s_out[tid >> 3] >> ((4 * tid) & 31)) & 15u;
    Cand c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float s = base + x[k];
        c[k] = (((out4 >> k) & 1u) || !(s > -INFINITY)) ? Cand{-INFINITY, NO_CAND} : Cand{s, v0 + k};
    }
    const size_t o0 = ((size_t)row * C + chunk) * b;
    select_rounds(c, b, s_v, s_i, cand_s + o0, cand_tok + o0);
}

__global__ __launch_bounds__(MERGE_T) void cbs_merge_kernel(const float *__restrict__ logp, const float *__restrict__ sums,
                                                            const int32_t *__restrict__ words, const int32_t *__restrict__ ncons,
                                                            const float *__restrict__ cand_s, const int *__restrict__ cand_tok,
                                                            int cur, int b, int S, int V1, int C, int force_end,
                                                            int32_t *__restrict__ parent, int64_t *__restrict__ token,
                                                            float *__restrict__ score, float *__restrict__ next_sums,
                                                            uint8_t *__restrict__ ended, uint8_t *__restrict__ valid) {
    __shared__ float l_s[CAND_MAX];
    __shared__ int l_i[CAND_MAX];                          // flat index row * V1 + token
    __shared__ float st_s[STAGE_MAX];
    __shared__ int st_i[STAGE_MAX];
    __shared__ int s_w[NW];
    __shared__ int s_n;
    const int tgt = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const int SB = S * b, per_row = C * b;
    const int nc = clamp_ncons(ncons[img], S);
    const float *sm = sums + (size_t)img * SB;
    // the rows that are in state tgt: the root is in state 0
    const int r0 = cur == 1 ? 0 : tgt * b, nrows = cur == 1 ? (tgt == 0 ? 1 : 0) : b;
    const int nstay = nrows * b, nmove = S > 1 ? cur * NW : 0, n = nstay + nmove;
    if (tid < NW) {
        const int v = words[(size_t)img * NW + tid];
        s_w[tid] = (tid / W_MAX < nc && v >= 0 && v < V1) ? v : -1;
    }
    if (tid == 0) s_n = 0;
    for (int e = tid; e < n; e += MERGE_T) {
        l_s[e] = -INFINITY;
        l_i[e] = NO_CAND;
    }
    // phase A: per row of the state, the b largest of its C chunk lists
    for (int j = 0; j < nrows; ++j) {
        const int r = r0 + j;
        if (!(sm[r] > -INFINITY)) continue;                // uniform: the row kernel wrote nothing for an empty slot
        const size_t src = ((size_t)img * cur + r) * per_row;
        __syncthreads();
        for (int e = tid; e < per_row; e += MERGE_T) {
            st_s[e] = cand_s[src + e];
            st_i[e] = cand_tok[src + e];
        }
        __syncthreads();
        best_of_lists<MERGE_T>(st_s, st_i, 1, per_row, b, l_s + j * b, l_i + j * b, r * V1);
    }
    __syncthreads();
    // phase B: the moving candidates, enumerated.  A token listed twice (one set twice, or two sets) is taken at its first listing.
    for (int e = tid; e < nmove; e += MERGE_T) {
        const int r = e / NW, w = e - r * NW;
        const int st = cur == 1 ? 0 : r / b;
        const int v = s_w[w];
        if (st == tgt || (st & ~tgt) || v < 0 || !(sm[r] > -INFINITY)) continue;
        int sat = 0, first = w;
        for (int w2 = NW - 1; w2 >= 0; --w2)
            if (s_w[w2] == v) {
                sat |= 1 << (w2 / W_MAX);
                first = w2;
            }
        if (first != w || (st | sat) != tgt) continue;
        const float s = sm[r] + logp[((size_t)img * cur + r) * V1 + v];
        if (!(s > -INFINITY)) continue;
        l_s[nstay + e] = s;
        l_i[nstay + e] = r * V1 + v;
    }
    __syncthreads();
    // phase C: the b largest, by counting
    const size_t o0 = (size_t)img * SB + tgt * b;
    best_of_candidates<MERGE_T>(
        l_s, l_i, n, b, &s_n,
        [&](int rank, int e) {
            const size_t o = o0 + rank;
            const float s = l_s[e];
            const int fl = l_i[e], par = fl / V1, tok = fl - par * V1;
            const bool end = tok == 0 || force_end;
            parent[o] = par;
            token[o] = tok;
            score[o] = s;
            next_sums[o] = end ? s - 1000.f : s;           // as capmi_beam_select
            ended[o] = end ? 1 : 0;
            valid[o] = 1;
        },
        [&](int slot) {
            const size_t o = o0 + slot;
            parent[o] = 0;
            token[o] = 0;
            score[o] = -INFINITY;
            next_sums[o] = -INFINITY;
            ended[o] = 0;
            valid[o] = 0;
        });
}

// one workgroup per image: every recorded (ended and valid) candidate gets the key (class, penalised score, step, slot), the
// best one is found by a block-wide reduction and thread 0 walks its parent pointers back
__global__ __launch_bounds__(FIN_T) void cbs_finalize_kernel(const int32_t *__restrict__ parent, const int64_t *__restrict__ token,
                                                            const float *__restrict__ score, const uint8_t *__restrict__ ended,
                                                            const uint8_t *__restrict__ valid, const int32_t *__restrict__ ncons,
                                                            const double *__restrict__ len_div, int B, int b, int S, int L,
                                                            int64_t *__restrict__ seq, int32_t *__restrict__ lineage,
                                                            int32_t *__restrict__ length, int32_t *__restrict__ state_out,
                                                            float *__restrict__ score_out) {
    __shared__ int s_cls[FIN_T];
    __shared__ double s_key[FIN_T];
    __shared__ int s_c[FIN_T];
    const int img = blockIdx.x, tid = threadIdx.x, SB = S * b, n = L * SB;
    const int full = (1 << clamp_ncons(ncons[img], S)) - 1;
    int bc = -1, bcls = -1;
    double bk = 0.0;
    for (int c = tid; c < n; c += FIN_T) {                 // ascending c = ascending (step, slot): a later equal key never wins
        const int t = c / SB, j = c - t * SB;
        const size_t o = ((size_t)t * B + img) * SB + j;
        if (!ended[o] || !valid[o]) continue;
        const int st = j / b;
        const int cls = st == full ? 1000 : __popc(st);
        const double s = (double)score[o];
        const double k = len_div ? s / len_div[t] : s;
        if (bc < 0 || cls > bcls || (cls == bcls && k > bk)) {
            bc = c;
            bcls = cls;
            bk = k;
        }
    }
    s_cls[tid] = bcls;
    s_key[tid] = bk;
    s_c[tid] = bc;
    __syncthreads();
    for (int w = FIN_T / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const int c2 = s_c[tid + w], c1 = s_c[tid];
            if (c2 >= 0) {
                const int cl1 = s_cls[tid], cl2 = s_cls[tid + w];
                const double k1 = s_key[tid], k2 = s_key[tid + w];
                if (c1 < 0 || cl2 > cl1 || (cl2 == cl1 && (k2 > k1 || (k2 == k1 && c2 < c1)))) {
                    s_c[tid] = c2;
                    s_cls[tid] = cl2;
                    s_key[tid] = k2;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int c = s_c[0];
        const int t = c >= 0 ? c / SB : -1;                // nothing recorded: an empty path
        const int slot = c - t * SB;
        length[img] = backtrack_path(parent, token, nullptr, B, SB, L, img, t, slot, seq + (size_t)img * L, lineage + img, B);
        state_out[img] = c >= 0 ? slot / b : 0;
        score_out[img] = c >= 0 ? (float)s_key[0] : 0.f;
    }
}

constexpr int LEAD = 3;                    // a row may start 3 floats into its first 16-byte piece
inline bool shape_ok(int B, int b, int S) {
    return B > 0 && b > 0 && S > 0 && S <= 16 && (S & (S - 1)) == 0 && (long long)S * b <= SB_MAX;
}

}  // namespace

extern "C" {

int64_t capmi_cbs_scratch_bytes(int B, int cur, int b, int V1) { return chunk_lists_bytes(B, cur, b, V1, LEAD); }

int capmi_cbs_select(const float *logp, const float *sums, const int32_t *words, const int32_t *ncons, int B, int cur, int b, int S,
                     int V1, int force_end, void *scratch, int64_t scratch_bytes, int32_t *parent, int64_t *token, float *score,
                     float *next_sums, uint8_t *ended, uint8_t *valid, void *stream) {
    if (!logp || !sums || !words || !ncons || !scratch || !parent || !token || !score || !next_sums || !ended || !valid)
        return CAPMI_EINVAL;
    if (!shape_ok(B, b, S) || V1 <= 0 || (cur != 1 && cur != S * b)) return CAPMI_EINVAL;
    const int C = chunks_of(V1, LEAD);
    ChunkLists cand;
    if ((long long)B * cur > 0x7fffffffLL || B > 65535 || C > 65535 || (long long)C * b > STAGE_MAX ||
        (long long)SB_MAX * V1 > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(logp) & 3))
        return CAPMI_EINVAL;
    if (!chunk_lists(scratch, scratch_bytes, B, cur, b, V1, LEAD, &cand)) return CAPMI_EINVAL;
    hipLaunchKernelGGL(cbs_row_kernel, dim3(B * cur, C), dim3(ROW_T), 0, (hipStream_t)stream, logp, sums, words, ncons, cur, b, S,
                       V1, C, cand.s, cand.tok);
    CAPMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(cbs_merge_kernel, dim3(S, B), dim3(MERGE_T), 0, (hipStream_t)stream, logp, sums, words, ncons, cand.s,
                       cand.tok, cur, b, S, V1, C, force_end, parent, token, score, next_sums, ended, valid);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_cbs_finalize(const int32_t *parent, const int64_t *token, const float *score, const uint8_t *ended, const uint8_t *valid,
                       const int32_t *ncons, const double *len_div, int B, int b, int S, int L, int64_t *seq, int32_t *lineage,
                       int32_t *length, int32_t *state, float *score_out, void *stream) {
    if (!parent || !token || !score || !ended || !valid || !ncons || !seq || !lineage || !length || !state || !score_out)
        return CAPMI_EINVAL;
    if (!shape_ok(B, b, S) || L <= 0 || (long long)L * S * b > FIN_MAX) return CAPMI_EINVAL;
    hipLaunchKernelGGL(cbs_finalize_kernel, dim3(B), dim3(FIN_T), 0, (hipStream_t)stream, parent, token, score, ended, valid, ncons,
                       len_div, B, b, S, L, seq, lineage, length, state, score_out);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
