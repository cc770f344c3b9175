// The search core that the beam search (beam.hip), the stochastic beam search (sbs.hip) and the constrained beam search (cbs.hip)
// share: the candidate order, the selection rounds of a row kernel, the two counting selections of a merge kernel, the walk back
// through the parent pointers, and the chunk-list scratch between a row kernel and its merge kernel.
//
// Order everywhere: the larger value first, equal values by the lower index (a token, or a flat index row * V1 + token), which is
// what torch.sort(stable) gives.  Nothing here depends on an arrival order: plain stores and integer counts only.
//
// The chunk-list scheme of sbs and cbs: a row kernel runs one workgroup of ROW_T threads per (search row, chunk of CHUNK floats);
// every thread holds one quad of candidates, and the chunk's b largest go, in order, to scratch.  The merge kernel then needs
// only the C * b listed candidates of a row, never the row itself.
#pragma once
#include "host_common.h"

namespace capmi {

constexpr int BD_MAX = 16;                 // beams per image of the beam search and of the stochastic beam search (ops.py SBS_BD_MAX)
constexpr int ROW_T = 256;                 // threads of a row-kernel workgroup
constexpr int CHUNK = 4 * ROW_T;           // floats of a row-kernel workgroup: one quad per thread

struct Cand {
    float v;
    int i;
};
constexpr int NO_CAND = 0x7fffffff;        // the index of an emptied list entry {-inf, NO_CAND}: it sorts behind every candidate

__device__ __forceinline__ bool before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }
// spelled out as a branch, not through before() or `? :`: with these very lines beam_select_kernel compiles to the code it always
// had; the `? :` form cost that kernel 13 %
__device__ __forceinline__ Cand best_of(Cand a, Cand b) {
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
    return a;
}
__device__ __forceinline__ void order2(Cand &a, Cand &b) {
    if (before(b.v, b.i, a.v, a.i)) {
        const Cand t = a;
        a = b;
        b = t;
    }
}
__device__ __forceinline__ Cand wave_best(Cand best) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = best_of(best, Cand{__shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64)});
    return best;
}

// The b largest of a ROW_T-thread workgroup's candidates, in order, to out_s / out_tok[0 .. b).  c: the thread's quad in any order
// (sorted here, best first; an entry that is no candidate is {-inf, anything}).  s_v / s_i: ROW_T / 64 words of LDS each.
// b rounds of wave shuffle, cross-wave LDS, and the thread that owns the winner pops it: indices of finite candidates are
// unique, so exactly one thread pops.  A -inf winner means that every list is empty; nobody pops, and the remaining rounds write
// that same entry again.  Which index such a -inf entry carries is the caller's business (cbs: NO_CAND; sbs: a real token), and no
// reader may depend on it: both merge kernels skip the -inf entries of a list.
__device__ __forceinline__ void select_rounds(Cand (&c)[4], int b, float *s_v, int *s_i, float *__restrict__ out_s,
                                              int *__restrict__ out_tok) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    order2(c[0], c[1]); order2(c[2], c[3]); order2(c[0], c[2]); order2(c[1], c[3]); order2(c[1], c[2]);
    for (int round = 0; round < b; ++round) {
        const Cand best = wave_best(c[0]);
        if (lane == 0) {
            s_v[wid] = best.v;
            s_i[wid] = best.i;
        }
        __syncthreads();
        Cand t{s_v[0], s_i[0]};
#pragma unroll
        for (int i = 1; i < ROW_T / 64; ++i) t = best_of(t, Cand{s_v[i], s_i[i]});
        if (threadIdx.x == 0) {
            out_s[round] = t.v;
            out_tok[round] = t.i;
        }
        if (t.v > -INFINITY && c[0].i == t.i) {
            c[0] = c[1]; c[1] = c[2]; c[2] = c[3];
            c[3] = Cand{-INFINITY, NO_CAND};
        }
        __syncthreads();                                   // s_v / s_i are rewritten next round
    }
}

// Phase A of a merge kernel: `rows` rows' chunk lists are staged in LDS, per_row = C * b entries (l_s, l_tok) each; the b largest
// of every row go, in order, to out_s / out_i[row * b + rank], the token plus `add`.  By counting: an entry's rank is the number of
// its row's entries in front of it.  -inf entries are skipped, so slots past a row's finite candidates keep what the caller put there.
template <int T>
__device__ __forceinline__ void best_of_lists(const float *l_s, const int *l_tok, int rows, int per_row, int b, float *out_s,
                                              int *out_i, int add) {
    for (int e = threadIdx.x; e < rows * per_row; e += T) {
        const float s = l_s[e];
        if (!(s > -INFINITY)) continue;
        const int jr = rows == 1 ? 0 : e / per_row, tok = l_tok[e], lo = jr * per_row;      // one row: no division once inlined
        int rank = 0;
        for (int e2 = lo; e2 < lo + per_row; ++e2) rank += before(l_s[e2], l_tok[e2], s, tok) ? 1 : 0;
        if (rank < b) {
            out_s[jr * b + rank] = s;
            out_i[jr * b + rank] = tok + add;
        }
    }
}

// Phase C of a merge kernel: the b largest of the n entries (v[e], i[e]) in LDS, by counting: store(rank, e) for the winners,
// fill(slot) for the slots past the number of candidates (fewer than b exist).  An entry that is no candidate is {-inf, NO_CAND}: it
// is in front of nothing, and only the index tells it from a candidate whose value is -inf.  s_n: one LDS word, zeroed by the
// caller before a barrier.  All threads of the workgroup call this.
template <int T, typename Store, typename Fill>
__device__ __forceinline__ void best_of_candidates(const float *v, const int *i, int n, int b, int *s_n, Store store, Fill fill) {
    int mine = 0;
    for (int e = threadIdx.x; e < n; e += T) {
        const int fl = i[e];
        if (fl == NO_CAND) continue;
        ++mine;
        const float s = v[e];
        int rank = 0;
        for (int e2 = 0; e2 < n; ++e2) rank += before(v[e2], i[e2], s, fl) ? 1 : 0;
        if (rank < b) store(rank, e);
    }
    if (mine) atomicAdd(s_n, mine);                        // an integer count: the order of arrival does not show
    __syncthreads();
    if ((int)threadIdx.x < b && (int)threadIdx.x >= *s_n) fill((int)threadIdx.x);
}

// One output path: from slot `slot` of step t, image img, back through the parent pointers of tables [L][B][W] (t < 0: no path).
// seq_row[s] gets the tokens; lineage_col[s * rows] the search row that produced step s's distribution -- img at step 0, where an
// image has one row, img * W + parent afterwards -- with the parent clamped into [0, W).  alive (or null): the path ends at its
// earliest step that is not alive; without it the path is t + 1 long.  Behind the end seq is padded with 0 and lineage with -1.
// Returns the length.
__device__ __forceinline__ int backtrack_path(const int32_t *__restrict__ parent, const int64_t *__restrict__ token,
                                              const uint8_t *__restrict__ alive, int B, int W, int L, int img, int t, int slot,
                                              int64_t *__restrict__ seq_row, int32_t *__restrict__ lineage_col, int rows) {
    int len = t + 1;
    for (int s = t; s >= 0; --s) {
        const size_t o = ((size_t)s * B + img) * W + slot;
        seq_row[s] = token[o];
        if (alive && !alive[o]) len = s + 1;
        int par = parent[o];
        par = par < 0 ? 0 : (par >= W ? W - 1 : par);
        lineage_col[(size_t)s * rows] = s == 0 ? img : img * W + par;
        slot = par;
    }
    for (int s = len; s < L; ++s) {
        seq_row[s] = 0;
        lineage_col[(size_t)s * rows] = -1;
    }
    return len;
}

// ---- host side: the chunk lists in scratch -- cand_s [rows][C][b] float, then cand_tok [rows][C][b] int32; rows = B * cur.
// lead: the floats a row may start into its first chunk (cbs cuts chunks on the row's own 16-byte grid: 3; sbs: 0)
inline int chunks_of(int V1, int lead) { return (V1 + lead + CHUNK - 1) / CHUNK; }

inline int64_t chunk_lists_bytes(int B, int cur, int b, int V1, int lead) {
    if (B <= 0 || cur <= 0 || b <= 0 || V1 <= 0) return 0;
    return (int64_t)B * cur * chunks_of(V1, lead) * b * 8;
}

struct ChunkLists {
    float *s;
    int *tok;
};

// false: the scratch is too small or off a 4-byte boundary
inline bool chunk_lists(void *scratch, int64_t scratch_bytes, int B, int cur, int b, int V1, int lead, ChunkLists *out) {
    if (scratch_bytes < chunk_lists_bytes(B, cur, b, V1, lead) || (reinterpret_cast<uintptr_t>(scratch) & 3)) return false;
    out->s = static_cast<float *>(scratch);
    out->tok = reinterpret_cast<int *>(out->s + (size_t)B * cur * chunks_of(V1, lead) * b);
    return true;
}

}  // namespace capmi
