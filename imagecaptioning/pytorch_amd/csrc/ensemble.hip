// Test-time ensemble (gfx950): the mixture log-probability of M members' rows.
// Reference: AttEnsemble.get_logprobs_state (AttEnsemble.py:45-53), log(sum_i w_i softmax(logit_i) / sum_i w_i), here in
// log space.  See include/capmi.h (capmi_ensemble_logprobs) for the contract and the edge cases.  The member rows are cut as row_sweep.h has
// it; both passes spell its sweep order out (see the kernel).
#include "host_common.h"
#include "lse_online.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int ENS_T = 256;             // 4 waves per row: 9.3 float4 per thread and member at V1 = 9488
constexpr int ENS_W = ENS_T / 64;

// what the launch needs, members with weight 0 already dropped (the array is indexed with unrolled constants only:
// a dynamically indexed kernel-argument array would be copied to scratch)
struct EnsArgs {
    const float *in[CAPMI_ENSEMBLE_MAX];
    float log_w[CAPMI_ENSEMBLE_MAX];
    float *out;
    int rows, V1, ld_in, ld_out;
    int vec;                           // every member's rows share one alignment mod 16 bytes: float4 body
};

// out = log sum_i exp(a_i) with a_i = (x_i - max_i) - c_i, c_i = log(sum_i) - log w_i, as m + log sum_i exp(a_i - m).
// x_i - max_i is exact for inputs near the row maximum (logits offset by 1e4 keep their digits); all a_i = -inf gives -inf.
template <int M>
__device__ __forceinline__ float mix(const float (&x)[M], const float (&mx)[M], const float (&c)[M]) {
    float a[M];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        a[i] = (x[i] - mx[i]) - c[i];
        m = fmaxf(m, a[i]);
    }
    const float base = m == -INFINITY ? 0.f : m;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < M; ++i) s += __expf(a[i] - base);
    return base + __logf(s);
}

template <int M>
__device__ __forceinline__ float mix_at(const float *const (&row)[M], int v, const float (&mx)[M], const float (&c)[M]) {
    float x[M];
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = row[i][v];
    return mix<M>(x, mx, c);
}

template <int M>
__global__ __launch_bounds__(ENS_T) void ensemble_logprobs_kernel(const EnsArgs e) {
    __shared__ float s_red[2 * M * ENS_W];
    const size_t r = blockIdx.x;
    const int V1 = e.V1, tid = threadIdx.x;
    const float *row[M];     // members share ld_in and their base alignment mod 16, so one per-row head aligns them all
#pragma unroll
    for (int i = 0; i < M; ++i) row[i] = e.in[i] + r * (size_t)e.ld_in;
    float *o = e.out + r * (size_t)e.ld_out;
    const RowSplit sp = row_split(row[0], V1, e.vec);        // the cut aligns member 0's row, hence all of them

    // Both passes spell sweep()'s order (body, head, tail) out: with the payloads in lambdas the kernels compile to other code,
    // M = 5 with two registers more, and at 50 rows M = 5, 6, 7 ran 1-2 % slower.
    // pass 1: per member online max and sum of exp over the row
    float m[M], s[M];
#pragma unroll
    for (int i = 0; i < M; ++i) m[i] = -INFINITY, s[i] = 0.f;
    for (int q = tid; q < sp.nv; q += ENS_T) {
        f32x4 x[M];
#pragma unroll
        for (int i = 0; i < M; ++i) x[i] = ld4(row[i] + sp.head + 4 * q);
#pragma unroll
        for (int i = 0; i < M; ++i) online4(m[i], s[i], x[i]);
    }
    for (int v = tid; v < sp.head; v += ENS_T)
#pragma unroll
        for (int i = 0; i < M; ++i) online1(m[i], s[i], row[i][v]);
    for (int v = sp.tail + tid; v < V1; v += ENS_T)
#pragma unroll
        for (int i = 0; i < M; ++i) online1(m[i], s[i], row[i][v]);
    block_lse<M, ENS_W>(m, s, s_red);
    float c[M];
#pragma unroll
    for (int i = 0; i < M; ++i) c[i] = __logf(s[i]) - e.log_w[i];

    // pass 2: re-read the member rows, write the mixture
    const bool out_vec = same16(o, row[0]);
    for (int q = tid; q < sp.nv; q += ENS_T) {
        f32x4 x[M];
#pragma unroll
        for (int i = 0; i < M; ++i) x[i] = ld4(row[i] + sp.head + 4 * q);
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float xk[M];
#pragma unroll
            for (int i = 0; i < M; ++i) xk[i] = x[i][k];
            y[k] = mix<M>(xk, m, c);
        }
        float *op = o + sp.head + 4 * q;
        if (out_vec) {
            st4(op, y);
        } else {
            op[0] = y.x; op[1] = y.y; op[2] = y.z; op[3] = y.w;
        }
    }
    for (int v = tid; v < sp.head; v += ENS_T) o[v] = mix_at<M>(row, v, m, c);
    for (int v = sp.tail + tid; v < V1; v += ENS_T) o[v] = mix_at<M>(row, v, m, c);
}

template <int M>
void launch(const EnsArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(ensemble_logprobs_kernel<M>, dim3(a.rows), dim3(ENS_T), 0, st, a);
}

}  // namespace

extern "C" int capmi_ensemble_logprobs(const capmi_ensemble *e, void *stream) {
    if (!e || e->M < 1 || e->M > CAPMI_ENSEMBLE_MAX || e->V1 <= 0 || e->rows < 0 || e->ld_in < e->V1 || e->ld_out < e->V1 || !e->out)
        return CAPMI_EINVAL;
    EnsArgs a{};
    a.out = e->out;
    a.rows = e->rows;
    a.V1 = e->V1;
    a.ld_in = e->ld_in;
    a.ld_out = e->ld_out;
    a.vec = 1;
    const size_t span_in = span(e->rows, e->ld_in, e->V1), span_out = span(e->rows, e->ld_out, e->V1);
    int n = 0;
    for (int i = 0; i < e->M; ++i) {
        const float w = e->w[i];
        if (!e->in[i] || !(w >= 0.f) || w == INFINITY) return CAPMI_EINVAL;      // (also NaN)
        if (!aligned4(e->in[i])) return CAPMI_EINVAL;
        if (overlaps(e->in[i], span_in, e->out, span_out)) return CAPMI_EINVAL;
        if (w == 0.f) continue;
        a.in[n] = e->in[i];
        a.log_w[n] = logf(w);
        if (!same_phase16(a.in[n], e->ld_in, a.in[0], e->ld_in)) a.vec = 0;
        ++n;
    }
    if (n == 0) return CAPMI_EINVAL;
    if (!aligned4(e->out)) return CAPMI_EINVAL;
    if (e->rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (n) {
        case 1: launch<1>(a, st); break;
        case 2: launch<2>(a, st); break;
        case 3: launch<3>(a, st); break;
        case 4: launch<4>(a, st); break;
        case 5: launch<5>(a, st); break;
        case 6: launch<6>(a, st); break;
        case 7: launch<7>(a, st); break;
        default: launch<8>(a, st); break;
    }
    CAPMI_CHECK_LAUNCH();
    return 0;
}
