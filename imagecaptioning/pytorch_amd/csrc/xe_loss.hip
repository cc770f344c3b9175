// Cross-entropy criteria of the teacher-forced pass (gfx950): LanguageModelCriterion (masked NLL) and LabelSmoothing (KL against
// the smoothed target distribution).  Reference: captioning/modules/losses.py:204-265.  See include/capmi.h (capmi_xe_loss_fwd /
// _bwd) for the contract.  Forward: stage 1 writes one value per (n, t) position -- a single gathered entry without smoothing
// (one thread per position), the row sum plus the gathered entry with smoothing (one workgroup per row, the row read once) --
// and stage 2, one workgroup, folds them in a fixed order (no atomics).  Backward: one elementwise launch over [N, T] that
// writes the sparse gradient (capmi_sparse_logp_grad); nothing dense is produced.
#include <math.h>

#include "host_common.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int XE_T = 256;              // 4 waves: 9.3 float4 per thread at V1 = 9488
constexpr int XE_W = XE_T / 64;

struct XeArgs {
    const float *logp;
    const int64_t *tok;
    const float *mask;
    float *pos, *msum, *loss;
    const float *g_out;
    float *g_sel, *g_sum;
    int N, T, V1, tok_ld, mask_ld, per_row;
    double off, cmo, ent;              // smoothing / (V1 - 1), confidence - off, sum_v q ln q
};

// logp[row, tok]; a token outside [0, V1) is not read and gives NaN
__device__ __forceinline__ float gather1(const float *lp, int64_t s, int V1) { return (s >= 0 && s < V1) ? lp[s] : __builtin_nanf(""); }

// smoothing == 0: pos[n, t] = -logp[n, t, tok] * mask, one thread per position; the dense row is not read
__global__ __launch_bounds__(XE_T) void xe_nll_kernel(const XeArgs a) {
    const int row = blockIdx.x * XE_T + threadIdx.x;
    if (row >= a.N * a.T) return;
    const int n = row / a.T, t = row - n * a.T;
    const float m = a.mask[(size_t)n * a.mask_ld + t];
    float v = 0.f;
    if (m != 0.f) v = -gather1(a.logp + (size_t)row * a.V1, a.tok[(size_t)n * a.tok_ld + t], a.V1) * m;
    a.pos[row] = v;
}

// smoothing > 0: pos[n, t] = (ent - off * sum_v logp[n, t, v] - (conf - off) * logp[n, t, tok]) * mask, one workgroup per row,
// the row cut and swept as row_sweep.h has it.
__global__ __launch_bounds__(XE_T) void xe_smooth_kernel(const XeArgs a) {
    __shared__ double s_red[XE_W];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int n = row / a.T, t = row - n * a.T;
    const float m = a.mask[(size_t)n * a.mask_ld + t];
    if (m == 0.f) {                                          // masked: nothing read, an exact 0
        if (tid == 0) a.pos[row] = 0.f;
        return;
    }
    const float *lp = a.logp + (size_t)row * a.V1;
    const int V1 = a.V1;
    const RowSplit sp = row_split(lp, V1, true);
    float sel = 0.f;                                         // loaded before the sweep, so its latency hides behind it
    if (tid == 0) sel = gather1(lp, a.tok[(size_t)n * a.tok_ld + t], V1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float edge = 0.f;
    sweep<XE_T>(sp, tid, [&](int v0) { acc += ld4(lp + v0); }, [&](int v) { edge += lp[v]; });
    // a thread holds at most a few terms per lane of `acc`; everything across threads is added in double, in a fixed tree
    double s[1] = {((double)acc.x + (double)acc.y) + ((double)acc.z + (double)acc.w) + (double)edge};
    if (!fold_d<1, XE_T>(s, s_red)) return;
    a.pos[row] = (float)(a.ent - (a.off * s[0] + a.cmo * (double)sel)) * m;
}

// stage 2: the masked means of one launch's positions.  Double accumulators, a fixed order: two runs are bit-equal.
__global__ __launch_bounds__(XE_T) void xe_fold_kernel(const XeArgs a) {
    __shared__ double s_red[2 * XE_W];
    const int tid = threadIdx.x;
    if (a.per_row) {                                         // 'none': each row's steps in order
        for (int n = tid; n < a.N; n += XE_T) {
            double sv = 0.0, sm = 0.0;
            for (int t = 0; t < a.T; ++t) {
                sv += a.pos[(size_t)n * a.T + t];
                sm += a.mask[(size_t)n * a.mask_ld + t];
            }
            a.msum[n] = (float)sm;
            a.loss[n] = (float)sv / (float)sm;               // an all-zero row: 0 / 0 = NaN, as the reference
        }
        return;
    }
    const int R = a.N * a.T;
    double s[2] = {0.0, 0.0};                                // value, mask
    for (int row = tid; row < R; row += XE_T) {
        const int n = row / a.T, t = row - n * a.T;
        s[0] += a.pos[row];
        s[1] += a.mask[(size_t)n * a.mask_ld + t];
    }
    if (!fold_d<2, XE_T>(s, s_red)) return;
    a.msum[0] = (float)s[1];
    a.loss[0] = (float)s[0] / (float)s[1];
}

// g_sel[n, t] = -(conf - off) * mask / msum * u,  g_sum[n, t] = -off * mask / msum * u  (u: the row's upstream value, or 1)
__global__ __launch_bounds__(XE_T) void xe_bwd_kernel(const XeArgs a) {
    const int row = blockIdx.x * XE_T + threadIdx.x;
    if (row >= a.N * a.T) return;
    const int n = row / a.T, t = row - n * a.T;
    const int k = a.per_row ? n : 0;
    const float m = a.mask[(size_t)n * a.mask_ld + t];
    float c = m / a.msum[k];
    if (a.g_out) c *= a.g_out[k];
    a.g_sel[row] = -(float)a.cmo * c;
    if (a.g_sum) a.g_sum[row] = -(float)a.off * c;
}

int common_args(const capmi_xe_loss *p, XeArgs &a) {
    if (!p || p->N <= 0 || p->T <= 0 || p->V1 <= 0 || p->tok_ld < p->T || p->mask_ld < p->T) return CAPMI_EINVAL;
    if (!(p->smoothing >= 0.0) || !(p->smoothing < 1.0)) return CAPMI_EINVAL;
    if (p->smoothing > 0.0 && p->V1 < 2) return CAPMI_EINVAL;               // no off-target entry to carry the mass
    if ((int64_t)p->N * p->T > 0x7fffffff) return CAPMI_EINVAL;
    if (!p->mask || !p->msum) return CAPMI_EINVAL;
    a = XeArgs{};
    a.logp = p->logp, a.tok = p->tok, a.mask = p->mask;
    a.pos = p->pos, a.msum = p->msum, a.loss = p->loss;
    a.g_out = p->g_out, a.g_sel = p->g_sel, a.g_sum = p->g_sum;
    a.N = p->N, a.T = p->T, a.V1 = p->V1, a.tok_ld = p->tok_ld, a.mask_ld = p->mask_ld;
    a.per_row = p->per_row ? 1 : 0;
    // the constants of (smoothing, V1) in double, handed to the kernels by value; a zero factor drops its term
    const double conf = 1.0 - p->smoothing;
    const double off = p->smoothing > 0.0 ? p->smoothing / (double)(p->V1 - 1) : 0.0;
    a.off = off;
    a.cmo = conf - off;
    a.ent = (double)(p->V1 - 1) * (off > 0.0 ? off * log(off) : 0.0) + (conf > 0.0 ? conf * log(conf) : 0.0);
    return 0;
}

}  // namespace

extern "C" int capmi_xe_loss_fwd(const capmi_xe_loss *p, void *stream) {
    XeArgs a;
    if (common_args(p, a) != 0) return CAPMI_EINVAL;
    if (!p->logp || !p->tok || !p->pos || !p->loss) return CAPMI_EINVAL;
    if (!aligned4(p->logp)) return CAPMI_EINVAL;
    const int R = p->N * p->T;
    hipStream_t st = (hipStream_t)stream;
    if (p->smoothing > 0.0)
        hipLaunchKernelGGL(xe_smooth_kernel, dim3(R), dim3(XE_T), 0, st, a);
    else
        hipLaunchKernelGGL(xe_nll_kernel, dim3((R + XE_T - 1) / XE_T), dim3(XE_T), 0, st, a);
    CAPMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(xe_fold_kernel, dim3(1), dim3(XE_T), 0, st, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_xe_loss_bwd(const capmi_xe_loss *p, void *stream) {
    XeArgs a;
    if (common_args(p, a) != 0) return CAPMI_EINVAL;
    if (!p->g_sel || (p->smoothing > 0.0 && !p->g_sum)) return CAPMI_EINVAL;
    if (!(p->smoothing > 0.0)) a.g_sum = nullptr;
    const int R = p->N * p->T;
    hipLaunchKernelGGL(xe_bwd_kernel, dim3((R + XE_T - 1) / XE_T), dim3(XE_T), 0, (hipStream_t)stream, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
