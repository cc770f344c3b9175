// Discriminative decoding (gfx950): the pragmatic row of a hypothesis from its decoder rows under the target image and under up
// to CAPMI_DISC_MAX - 1 distractor images (Vedantam et al. 2017, the emitter-suppressor speaker; Cohn-Gordon et al. 2018, the
// listener form).  See include/capmi.h (capmi_disc_combine) for the contract and the edge cases.  One workgroup per hypothesis,
// two sweeps over its slot rows: the rows are cut as row_sweep.h has it, the running logsumexp is lse_online.h's (ensemble.hip's);
// both passes spell the sweep order out, as ensemble_logprobs_kernel does and for its reason.
#include "host_common.h"
#include "lse_online.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int DISC_T = 256;            // 4 waves per hypothesis: 9.3 float4 per thread and slot at V1 = 9488
constexpr int DISC_W = DISC_T / 64;

struct DiscArgs {
    const float *in;
    const uint8_t *present;
    float *out;
    int D1, cur, V1, ld_in, ld_out;
    float w;                           // 1 - lambda
    int vec;                           // the slot rows of a hypothesis share one alignment mod 16 bytes: float4 body
};

// One column.  x: the slots' logits (0 where a slot is absent), mx / c: the rows' max and log sum exp(x - max), so that
// (x_i - mx_i) - c_i is slot i's log-probability (exact differences near the row maximum, as in ensemble.hip's mix).
//   suppress: u = lt - w (logsumexp_{i >= 1 present} l_i - log D')
//   listener: u = lt + w (lt - logsumexp_{i present, the target included} l_i)
// The logsumexp runs in log space, m + log sum exp(a_i - m); all a_i = -inf gives -inf (suppress: u = +inf).  lt = -inf gives
// -inf whatever the distractors say; a NaN in any present slot reaches u.
template <int M, bool LISTENER>
__device__ __forceinline__ float combine(const float (&x)[M], const float (&mx)[M], const float (&c)[M], unsigned mask, float w,
                                         float log_d) {
    const float lt = (x[0] - mx[0]) - c[0];
    float a[M];
    float m = -INFINITY;
#pragma unroll
    for (int i = LISTENER ? 0 : 1; i < M; ++i) {
        a[i] = (mask >> i) & 1u ? (x[i] - mx[i]) - c[i] : -INFINITY;
        m = fmaxf(m, a[i]);
    }
    const float base = m == -INFINITY ? 0.f : m;
    float s = 0.f;
#pragma unroll
    for (int i = LISTENER ? 0 : 1; i < M; ++i) s += __expf(a[i] - base);
    const float lse = base + __logf(s);
    const float u = LISTENER ? lt + w * (lt - lse) : lt - w * (lse - log_d);
    return lt == -INFINITY ? -INFINITY : u;
}

template <int M, bool LISTENER>
__global__ __launch_bounds__(DISC_T) void disc_combine_kernel(const DiscArgs e) {
    __shared__ float s_red[2 * M * DISC_W];
    const int b = blockIdx.x / e.cur, j = blockIdx.x - b * e.cur;
    const int V1 = e.V1, tid = threadIdx.x;
    // the present slots of this image as a bit mask (uniform over the workgroup); the target always; w == 0: the target alone
    unsigned mask = 1u;
    if (e.w != 0.f) {
#pragma unroll
        for (int i = 1; i < M; ++i) mask |= e.present[(size_t)b * M + i] ? 1u << i : 0u;
    }
    const float *row[M];     // inner row (b * D1 + i) * cur + j; the launcher's vec says one cut aligns them all
#pragma unroll
    for (int i = 0; i < M; ++i) row[i] = e.in + (((size_t)b * M + i) * e.cur + j) * (size_t)e.ld_in;
    float *o = e.out + (size_t)blockIdx.x * e.ld_out;
    const bool only = mask == 1u;
    const RowSplit sp = row_split(row[0], V1, e.vec || only);
    const bool out_vec = same16(o, row[0]);

    // pass 1: per present slot the online max and sum of exp over the row; an absent slot keeps (-inf, 0) and is not read
    float m[M], s[M];
#pragma unroll
    for (int i = 0; i < M; ++i) m[i] = -INFINITY, s[i] = 0.f;
    for (int q = tid; q < sp.nv; q += DISC_T) {
        f32x4 x[M];
#pragma unroll
        for (int i = 0; i < M; ++i)
            if ((mask >> i) & 1u) x[i] = ld4(row[i] + sp.head + 4 * q);
#pragma unroll
        for (int i = 0; i < M; ++i)
            if ((mask >> i) & 1u) online4(m[i], s[i], x[i]);
    }
    for (int v = tid; v < sp.head; v += DISC_T)
#pragma unroll
        for (int i = 0; i < M; ++i)
            if ((mask >> i) & 1u) online1(m[i], s[i], row[i][v]);
    for (int v = sp.tail + tid; v < V1; v += DISC_T)
#pragma unroll
        for (int i = 0; i < M; ++i)
            if ((mask >> i) & 1u) online1(m[i], s[i], row[i][v]);
    block_lse<M, DISC_W>(m, s, s_red);
    float c[M];
#pragma unroll
    for (int i = 0; i < M; ++i) c[i] = __logf(s[i]);

    if (only) {
        // no distractor, or lambda = 1: the target's log_softmax
        for (int q = tid; q < sp.nv; q += DISC_T) {
            const f32x4 x = ld4(row[0] + sp.head + 4 * q);
            f32x4 y;
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = (x[k] - m[0]) - c[0];
            float *op = o + sp.head + 4 * q;
            if (out_vec) {
                st4(op, y);
            } else {
                op[0] = y.x; op[1] = y.y; op[2] = y.z; op[3] = y.w;
            }
        }
        for (int v = tid; v < sp.head; v += DISC_T) o[v] = (row[0][v] - m[0]) - c[0];
        for (int v = sp.tail + tid; v < V1; v += DISC_T) o[v] = (row[0][v] - m[0]) - c[0];
        return;
    }

    // pass 2: re-read the present rows (from L2: at most 8 x 38 KB at V1 = 9488), write u
    const float w = e.w, log_d = __logf((float)(__popc(mask) - 1));
    for (int q = tid; q < sp.nv; q += DISC_T) {
        f32x4 x[M];
#pragma unroll
        for (int i = 0; i < M; ++i) x[i] = (mask >> i) & 1u ? ld4(row[i] + sp.head + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float xk[M];
#pragma unroll
            for (int i = 0; i < M; ++i) xk[i] = x[i][k];
            y[k] = combine<M, LISTENER>(xk, m, c, mask, w, log_d);
        }
        float *op = o + sp.head + 4 * q;
        if (out_vec) {
            st4(op, y);
        } else {
            op[0] = y.x; op[1] = y.y; op[2] = y.z; op[3] = y.w;
        }
    }
    auto edge = [&](int v) {
        float xk[M];
#pragma unroll
        for (int i = 0; i < M; ++i) xk[i] = (mask >> i) & 1u ? row[i][v] : 0.f;
        o[v] = combine<M, LISTENER>(xk, m, c, mask, w, log_d);
    };
    for (int v = tid; v < sp.head; v += DISC_T) edge(v);
    for (int v = sp.tail + tid; v < V1; v += DISC_T) edge(v);
}

template <int M>
void launch(const DiscArgs &a, int rows, int listener, hipStream_t st) {
    if (listener)
        hipLaunchKernelGGL((disc_combine_kernel<M, true>), dim3(rows), dim3(DISC_T), 0, st, a);
    else
        hipLaunchKernelGGL((disc_combine_kernel<M, false>), dim3(rows), dim3(DISC_T), 0, st, a);
}

}  // namespace

extern "C" int capmi_disc_combine(const capmi_disc *d, void *stream) {
    if (!d || d->D1 < 1 || d->D1 > CAPMI_DISC_MAX || d->B < 0 || d->cur < 0 || d->V1 <= 0 || d->ld_in < d->V1 || d->ld_out < d->V1)
        return CAPMI_EINVAL;
    if (d->mode != 0 && d->mode != 1) return CAPMI_EINVAL;
    if (!(d->lambda >= 0.f && d->lambda <= 1.f)) return CAPMI_EINVAL;      // (also NaN)
    if (!d->in || !d->present || !d->out || !aligned4(d->in, d->out)) return CAPMI_EINVAL;
    const int64_t rows = (int64_t)d->B * d->cur, rows_in = rows * d->D1;
    if (rows_in > INT32_MAX) return CAPMI_EINVAL;
    if (overlaps(d->in, span((int)rows_in, d->ld_in, d->V1), d->out, span((int)rows, d->ld_out, d->V1))) return CAPMI_EINVAL;
    if (rows == 0) return 0;
    DiscArgs a{};
    a.in = d->in;
    a.present = d->present;
    a.out = d->out;
    a.D1 = d->D1;
    a.cur = d->cur;
    a.V1 = d->V1;
    a.ld_in = d->ld_in;
    a.ld_out = d->ld_out;
    a.w = 1.f - d->lambda;
    // slot i of a hypothesis lies i * cur rows behind slot 0: one cut of a row aligns every slot when those rows share their phase.
    // The output row's phase is compared in the kernel, row by row (its row index is not the slots').
    a.vec = 1;
    for (int i = 1; i < d->D1; ++i)
        if (!same_phase16(d->in + (size_t)i * d->cur * d->ld_in, d->ld_in, d->in, d->ld_in)) a.vec = 0;
    hipStream_t st = (hipStream_t)stream;
    switch (d->D1) {
        case 1: launch<1>(a, (int)rows, d->mode, st); break;
        case 2: launch<2>(a, (int)rows, d->mode, st); break;
        case 3: launch<3>(a, (int)rows, d->mode, st); break;
        case 4: launch<4>(a, (int)rows, d->mode, st); break;
        case 5: launch<5>(a, (int)rows, d->mode, st); break;
        case 6: launch<6>(a, (int)rows, d->mode, st); break;
        case 7: launch<7>(a, (int)rows, d->mode, st); break;
        default: launch<8>(a, (int)rows, d->mode, st); break;
    }
    CAPMI_CHECK_LAUNCH();
    return 0;
}
