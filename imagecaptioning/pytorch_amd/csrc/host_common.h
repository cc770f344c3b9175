// Host-side helpers shared by the native drivers and launchers of libcapmi.  Internal: not part of the C ABI in
// include/capmi.h.
#pragma once
#include "capmi_common.h"
#include "../../../include/capmi.h"

// return a nonzero status (CAPMI_* or hipError_t) to the caller
#define RC(x)                 \
    do {                      \
        int rc__ = (x);       \
        if (rc__) return rc__;\
    } while (0)

// the same for calls that return a hipError_t (memsets, copies)
#define HIP_RC(x)                                 \
    do {                                          \
        hipError_t e__ = (x);                     \
        if (e__ != hipSuccess) return (int)e__;   \
    } while (0)

// workgroups of a grid-stride launch over `work` items
inline int grid_for(size_t work, int per_block = 256, int cap = 2048) {
    size_t b = (work + per_block - 1) / per_block;
    if (b > (size_t)cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// all (possibly null) pointers 16-byte aligned
template <typename... P>
inline bool aligned16(P... p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

// all (possibly null) pointers 4-byte aligned
template <typename... P>
inline bool aligned4(P... p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 3) == 0;
}

// bytes from the first to past the last element of a [rows, V1] float matrix of leading dimension ld
inline size_t span(int rows, int ld, int V1) { return ((size_t)(rows > 0 ? rows - 1 : 0) * ld + V1) * sizeof(float); }

// the byte ranges [a, a + na) and [b, b + nb) meet
inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
    return pa < pb + nb && pb < pa + na;
}

// every row of p (leading dimension ld_p floats) sits at the same offset mod 16 bytes as the same row of q: one cut of a row
// (row_sweep.h) aligns both, so a kernel may sweep them with float4
inline bool same_phase16(const void *p, int64_t ld_p, const void *q, int64_t ld_q) {
    return ((reinterpret_cast<uintptr_t>(p) ^ reinterpret_cast<uintptr_t>(q)) & 15) == 0 && (ld_p - ld_q) % 4 == 0;
}

// one K segment of a capmi_gemm_f32 call; a_row_div <= 0 means 1
struct SegSpec {
    const float *A;
    int lda;
    const float *B;
    int ldb;
    int K;
    int a_row_div;
    const void *Apl;        // the same activations as A planes (capmi.h capmi_planes_from_f32), or null
};

// one column segment of a [K][N] B that is read in place (capmi_gemm_desc.n_bcol)
struct BColSpec {
    const float *B;
    int ldb, ncol;
};

// C[M,N] = sum_s A_s op B_s ; thin wrapper filling capmi_gemm_desc.  The segments' A planes are used only with zero_planes.
inline int gemm(void *stream, int a_layout, int b_layout, int M, int N, float *C, int ldc, const SegSpec *segs, int nseg,
                float *partial, int64_t cap, int defer, int *splits_used, const float *bias = nullptr,
                const float *bias2 = nullptr, int accumulate = 0, const void *zero_planes = nullptr, int splits_hint = 0,
                const BColSpec *bcols = nullptr, int nbcol = 0) {
    capmi_gemm_desc d{};
    d.nseg = nseg;
    for (int i = 0; i < nseg; ++i) {
        d.seg[i].A = segs[i].A; d.seg[i].lda = segs[i].lda;
        d.seg[i].B = segs[i].B; d.seg[i].ldb = segs[i].ldb;
        d.seg[i].K = segs[i].K; d.seg[i].a_row_div = segs[i].a_row_div > 0 ? segs[i].a_row_div : 1;
        d.a_planes[i] = zero_planes ? segs[i].Apl : nullptr;
    }
    d.a_layout = a_layout; d.b_layout = b_layout;
    d.M = M; d.N = N; d.C = C; d.ldc = ldc;
    d.bias = bias; d.bias2 = bias2;
    d.accumulate = accumulate;
    d.partial = partial; d.partial_capacity = cap;
    d.splits = splits_hint; d.defer_reduce = defer;
    d.n_bcol = nbcol;
    for (int i = 0; i < nbcol && i < CAPMI_MAX_BCOL; ++i) { d.bcol_B[i] = bcols[i].B; d.bcol_ldb[i] = bcols[i].ldb; d.bcol_n[i] = bcols[i].ncol; }
    const int rc = capmi_gemm_f32(&d, stream);
    if (splits_used) *splits_used = d.splits_used;
    return rc;
}

// d(logits) [T,N,V1] of a rollout's backward.  raw: the rollout returned logits, so d(logits) is the loss gradient itself
// (sparse and / or dense part), no softmax Jacobian.
inline int dlogits_bwd(bool raw, const capmi_sparse_logp_grad *sparse, const float *g_seq_logp, const float *seq_logp,
                       const uint8_t *live, float *dlogits, int N, int L, int T, int V1, void *stream) {
    if (raw) {
        capmi_sparse_logp_grad sp = sparse ? *sparse : capmi_sparse_logp_grad{};
        sp.raw = 1;
        return capmi_logsoftmax_bwd_sparse(&sp, g_seq_logp, seq_logp, live, dlogits, N, L, T, V1, stream);
    }
    if (sparse) return capmi_logsoftmax_bwd_sparse(sparse, g_seq_logp, seq_logp, live, dlogits, N, L, T, V1, stream);
    return capmi_logsoftmax_bwd(g_seq_logp, seq_logp, live, dlogits, N, L, T, V1, stream);
}
