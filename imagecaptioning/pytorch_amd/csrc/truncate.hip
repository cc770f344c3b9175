// Truncation samplers (gfx950): min-p, epsilon and eta sampling (Hewitt et al. 2022) and locally typical sampling (Meister et al.
// 2022) as one vocabulary-row kernel in front of capmi_select_logp.  See include/capmi.h (capmi_truncate_rows) for the rules and the
// contract.  One workgroup of 16 wave64s per row, the row cut and swept as row_sweep.h has it.  Passes over a row:
//   1  m = max x / T
//   2  S = sum e^(z), A = sum e^(z) (-z) with z = x / T - m: log-sum-exp and entropy H = log S + A / S in one pass (double folds)
//   T  typical only: 31-step radix descent over the bits of the score s = |(log S - z) - H| (a non-negative float orders as its bit
//      pattern), one block-wide mass sum per bit -- the descent of the nucleus filter in sampler.hip on another key
//   3  the kept mass and count under the threshold (double folds)
//   4  q = z - log(kept mass) on the kept set, -inf elsewhere; the store row
// Every decision is taken in the log domain relative to the row maximum: z >= log a (min-p), z >= log e + log S (epsilon),
// z >= min(log e, log e / 2 - H) + log S (eta); z == 0 is the maximum itself, which epsilon and eta always keep.
// Two arms, one body: Row<NQ> keeps the float4 groups of the row in registers (NQ = 1..3 groups per thread, V1 <= 12288, rows on 16-byte
// boundaries), Row<0> re-reads them in every pass.  Both hand the payloads the same values in the same order, and the file is built
// without fma contraction, so on one row the arms agree bit for bit.
#include "host_common.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int TR_T = 1024;
constexpr int TR_W = TR_T / 64;
constexpr int TR_REG_V1 = 3 * 4 * TR_T;      // 12288: three float4 per thread

struct TruncArgs {
    const float *logp;
    float *q, *kept_mass, *store;
    int *kept;
    const uint8_t *unfinished;
    int64_t store_ld;
    int ld, ld_q, V1, kind;
    float tau, lparam, invT;               // tau: the mass of typical sampling; lparam: log of the parameter of the other rules
};

template <int NQ>
struct Row {
    const float *p;
    RowSplit sp;
    f32x4 x[NQ ? NQ : 1];

    __device__ __forceinline__ void load(int tid) {
        if (NQ) {
#pragma unroll
            for (int j = 0; j < (NQ ? NQ : 1); ++j) {
                const int g = tid + j * TR_T;
                x[j] = g < sp.nv ? ld4(p + sp.head + 4 * g) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
    }
    // row_sweep.h's order for thread tid: its float4 groups, then its share of the head, then of the tail
    template <class F4, class F1>
    __device__ __forceinline__ void each4(int tid, F4 body4, F1 edge1) const {
        if (NQ) {
#pragma unroll
            for (int j = 0; j < (NQ ? NQ : 1); ++j) {
                const int g = tid + j * TR_T;
                if (g < sp.nv) body4(x[j], sp.head + 4 * g);
            }
        } else {
            for (int g = tid; g < sp.nv; g += TR_T) body4(ld4(p + sp.head + 4 * g), sp.head + 4 * g);
        }
        for (int v = tid; v < sp.head; v += TR_T) edge1(p[v], v);
        for (int v = sp.tail + tid; v < sp.V1; v += TR_T) edge1(p[v], v);
    }
    template <class F>
    __device__ __forceinline__ void each(int tid, F f) const {
        each4(
            tid,
            [&](f32x4 v, int) {
#pragma unroll
                for (int k = 0; k < 4; ++k) f(v[k]);
            },
            [&](float v, int) { f(v); });
    }
};

// s[0..K) summed over the workgroup in fold_d's fixed tree and handed to every thread
template <int K>
__device__ __forceinline__ void fold_all(double (&s)[K], double *lds) {
    if (fold_d<K, TR_T>(s, lds)) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[K * TR_W + k] = s[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = lds[K * TR_W + k];
    __syncthreads();       // the slots are free for the next fold
}

template <int NQ>
__global__ __launch_bounds__(TR_T) void truncate_rows_kernel(const TruncArgs a) {
    __shared__ float s_f[32];
    __shared__ double s_d[2 * TR_W + 2];
    const int r = blockIdx.x, tid = threadIdx.x;
    Row<NQ> row;
    row.p = a.logp + (size_t)r * a.ld;
    row.sp = row_split(row.p, a.V1, true);
    row.load(tid);
    const float invT = a.invT;
    const bool typ = a.kind == CAPMI_TRUNCATE_TYP;

    // pass 1
    float m = -INFINITY;
    row.each(tid, [&](float x) { m = fmaxf(m, x * invT); });
    m = block_max(m, s_f);

    // pass 2
    float fs = 0.f, fa = 0.f;
    row.each(tid, [&](float x) {
        const float z = x * invT - m;
        const float e = __expf(z);
        fs += e;
        fa += z == -INFINITY ? 0.f : e * -z;
    });
    double d[2] = {(double)fs, (double)fa};
    fold_all<2>(d, s_d);
    const double S = d[0];
    const float logS = (float)log(S), H = (float)(log(S) + d[1] / S);

    // the threshold on z (the other rules), or on the score's bits (typical)
    float thr = -INFINITY;
    uint32_t cut = 0;
    if (a.kind == CAPMI_TRUNCATE_MINP) thr = a.lparam;
    else if (a.kind == CAPMI_TRUNCATE_EPS) thr = a.lparam + logS;
    else if (a.kind == CAPMI_TRUNCATE_ETA) thr = fminf(a.lparam, 0.5f * a.lparam - H) + logS;
    else {
        // cut = the smallest key whose mass{key <= cut} reaches tau: bit by bit, the answer is >= cand while the mass below cand is short
        const float target = a.tau * (float)S;
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = cut | (1u << bit);
            float acc = 0.f;
            row.each(tid, [&](float x) {
                const float z = x * invT - m;
                acc += f2u(fabsf((logS - z) - H)) < cand ? __expf(z) : 0.f;
            });
            acc = block_sum(acc, s_f);
            if (acc < target) cut = cand;
        }
    }
    auto keeps = [&](float z) {
        if (typ) return z != -INFINITY && f2u(fabsf((logS - z) - H)) <= cut;
        return z >= thr || z == 0.f;
    };

    // pass 3
    float fk = 0.f, fn = 0.f;
    row.each(tid, [&](float x) {
        const float z = x * invT - m;
        if (keeps(z)) {
            fk += __expf(z);
            fn += 1.f;
        }
    });
    d[0] = (double)fk;
    d[1] = (double)fn;
    fold_all<2>(d, s_d);
    const float logK = (float)log(d[0]);
    if (tid == 0) {
        if (a.kept) a.kept[r] = (int)d[1];
        if (a.kept_mass) a.kept_mass[r] = (float)(d[0] / S);
    }

    // pass 4
    float *qr = a.q + (size_t)r * a.ld_q;
    float *sr = a.store ? a.store + (size_t)r * a.store_ld : nullptr;
    const bool q_vec = same16(qr, row.p), s_vec = sr && same16(sr, row.p);
    const bool unf = a.unfinished ? a.unfinished[r] != 0 : true;
    auto out1 = [&](float x) {
        const float z = x * invT - m;
        return keeps(z) ? z - logK : -INFINITY;
    };
    auto keep1 = [&](float x) { return unf ? x : x * 0.f; };
    row.each4(
        tid,
        [&](f32x4 x, int v0) {
            const f32x4 y = {out1(x[0]), out1(x[1]), out1(x[2]), out1(x[3])};
            if (q_vec) {
                st4(qr + v0, y);
            } else {
                qr[v0] = y[0]; qr[v0 + 1] = y[1]; qr[v0 + 2] = y[2]; qr[v0 + 3] = y[3];
            }
            if (sr) {
                const f32x4 w = {keep1(x[0]), keep1(x[1]), keep1(x[2]), keep1(x[3])};
                if (s_vec) {
                    st4(sr + v0, w);
                } else {
                    sr[v0] = w[0]; sr[v0 + 1] = w[1]; sr[v0 + 2] = w[2]; sr[v0 + 3] = w[3];
                }
            }
        },
        [&](float x, int v) {
            qr[v] = out1(x);
            if (sr) sr[v] = keep1(x);
        });
}

}  // namespace

extern "C" int capmi_truncate_rows(const float *logp, int ld, float *q, int ld_q, int N, int V1, int kind, float param,
                                   float temperature, int *kept, float *kept_mass, float *store, int64_t store_ld,
                                   const uint8_t *unfinished, void *stream) {
    const bool force_stream = (kind & CAPMI_TRUNCATE_STREAM) != 0;
    kind &= ~CAPMI_TRUNCATE_STREAM;
    if (!logp || !q || N < 0 || V1 <= 0 || ld < V1 || ld_q < V1 || !aligned4(logp, q, kept, kept_mass, store)) return CAPMI_EINVAL;
    if (kind < CAPMI_TRUNCATE_MINP || kind > CAPMI_TRUNCATE_TYP) return CAPMI_EINVAL;
    if (!(temperature > 0.f) || !(param > 0.f)) return CAPMI_EINVAL;                       // (also NaN)
    if (kind == CAPMI_TRUNCATE_MINP ? !(param <= 1.f) : !(param < 1.f)) return CAPMI_EINVAL;
    if (store && store_ld < V1) return CAPMI_EINVAL;
    if (N == 0) return 0;
    if (overlaps(logp, span(N, ld, V1), q, span(N, ld_q, V1))) return CAPMI_EINVAL;
    if (store) {
        const size_t sb = ((size_t)(N - 1) * (size_t)store_ld + V1) * sizeof(float);
        if (overlaps(store, sb, logp, span(N, ld, V1)) || overlaps(store, sb, q, span(N, ld_q, V1))) return CAPMI_EINVAL;
    }
    TruncArgs a{};
    a.logp = logp;
    a.q = q;
    a.kept = kept;
    a.kept_mass = kept_mass;
    a.store = store;
    a.unfinished = unfinished;
    a.store_ld = store_ld;
    a.ld = ld;
    a.ld_q = ld_q;
    a.V1 = V1;
    a.kind = kind;
    a.tau = param;
    a.lparam = (float)log((double)param);
    a.invT = 1.f / temperature;
    hipStream_t st = (hipStream_t)stream;
    const bool reg = !force_stream && V1 <= TR_REG_V1 && aligned16(logp) && (N == 1 || ld % 4 == 0);
    const int nv = V1 >> 2;
    if (!reg) hipLaunchKernelGGL(truncate_rows_kernel<0>, dim3(N), dim3(TR_T), 0, st, a);
    else if (nv <= TR_T) hipLaunchKernelGGL(truncate_rows_kernel<1>, dim3(N), dim3(TR_T), 0, st, a);
    else if (nv <= 2 * TR_T) hipLaunchKernelGGL(truncate_rows_kernel<2>, dim3(N), dim3(TR_T), 0, st, a);
    else hipLaunchKernelGGL(truncate_rows_kernel<3>, dim3(N), dim3(TR_T), 0, st, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
