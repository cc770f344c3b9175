// Knowledge distillation loss (gfx950): hard-label NLL mixed with the temperature-softened KL(teacher || student) of the
// teacher-forced pass.  No reference counterpart; see include/capmi.h (capmi_distill_loss_fwd / _bwd) for the normative formula and
// the edge cases.  Forward: one workgroup per (i, t) row reads the student and the teacher row once, in one sweep, then one
// workgroup folds the masked means in double.  Backward: one workgroup per row reads both rows once and writes the dense gradient
// once (plain stores: the teacher-forced backward reads it next).  Rows are cut and swept, and the means folded, as row_sweep.h has
// it; a teacher row is addressed through t_rows, so whether a row pair shares its alignment is decided per row, in the kernel.
#include <float.h>
#include <math.h>

#include "host_common.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int KD_T = 256;              // 4 waves per row: 9.3 float4 per thread and row at V1 = 9488 (the PPO row shape)
constexpr int FIN_T = 1024;

struct KdArgs {
    const float *lp_s, *lp_t;
    const int64_t *tok;
    const float *mask;
    float *lse_s, *lse_t, *kl, *nll;   // the four planes of row_stats
    float *msum, *out, *loss_rows;
    const float *g_out;
    float *grad;
    int N, T, V1, ld_s, ld_t, ld_grad, t_rows, tok_ld, mask_ld, per_row;
    float lambda, tau, inv_tau;
};

// the running state of one thread's share of a row pair: max and sum of e^(x - max) for the tempered student (A) and teacher (B)
// rows, and sum e^(b - maxB) (b - a).  The maxima start at -FLT_MAX, not -inf, so that a -inf entry rescales by e^0.
struct Run {
    float mA = -FLT_MAX, sA = 0.f, mB = -FLT_MAX, sB = 0.f, acc = 0.f;
};

// e^(b - mB) (b - a); a teacher entry of probability 0 contributes an exact 0 (not 0 * inf)
__device__ __forceinline__ float kl_term(float e, float a, float b) { return e > 0.f ? e * (b - a) : 0.f; }

__device__ __forceinline__ void push1(Run &r, float a, float b) {
    const float nA = fmaxf(r.mA, a), nB = fmaxf(r.mB, b);
    const float fB = __expf(r.mB - nB), e = __expf(b - nB);
    r.sA = r.sA * __expf(r.mA - nA) + __expf(a - nA);
    r.sB = r.sB * fB + e;
    r.acc = r.acc * fB + kl_term(e, a, b);
    r.mA = nA, r.mB = nB;
}

__device__ __forceinline__ void push4(Run &r, f32x4 a, f32x4 b) {
    const float nA = fmaxf(r.mA, fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)));
    const float nB = fmaxf(r.mB, fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
    const float fB = __expf(r.mB - nB);
    const float e0 = __expf(b.x - nB), e1 = __expf(b.y - nB), e2 = __expf(b.z - nB), e3 = __expf(b.w - nB);
    r.sA = r.sA * __expf(r.mA - nA) + ((__expf(a.x - nA) + __expf(a.y - nA)) + (__expf(a.z - nA) + __expf(a.w - nA)));
    r.sB = r.sB * fB + ((e0 + e1) + (e2 + e3));
    r.acc = r.acc * fB + ((kl_term(e0, a.x, b.x) + kl_term(e1, a.y, b.y)) + (kl_term(e2, a.z, b.z) + kl_term(e3, a.w, b.w)));
    r.mA = nA, r.mB = nB;
}

__global__ __launch_bounds__(KD_T) void distill_rows_kernel(const KdArgs a) {
    __shared__ float s_red[32];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int i = row / a.T, t = row - i * a.T;
    const float m = a.mask[(size_t)i * a.mask_ld + t];
    if (m == 0.f) {                                          // masked: nothing read (capmi.h)
        if (tid == 0) a.lse_s[row] = 0.f, a.lse_t[row] = 0.f, a.kl[row] = 0.f, a.nll[row] = 0.f;
        return;
    }
    const float *ls = a.lp_s + (size_t)row * a.ld_s;
    const float *lt = a.lp_t + ((size_t)i * a.t_rows + t) * a.ld_t;
    const int V1 = a.V1;
    const RowSplit sp = row_split(ls, V1, same16(ls, lt));
    // the target's entry: loaded before the sweep, so its latency hides behind it
    float nll = 0.f;
    if (tid == 0) {
        const int64_t s = a.tok[(size_t)i * a.tok_ld + t];
        nll = (s >= 0 && s < V1) ? -ls[s] : __builtin_nanf("");
    }
    const float it = a.inv_tau;
    Run r;
    // sweep()'s order, written out: with the payload in lambdas this kernel compiles to other code (by reference x * it is fused
    // into push4's b - a, an fma with other bits; by value it costs a register)
    for (int q = tid; q < sp.nv; q += KD_T) {
        const f32x4 x = ld4(ls + sp.head + 4 * q), y = ld4(lt + sp.head + 4 * q);
        push4(r, x * it, y * it);
    }
    for (int v = tid; v < sp.head; v += KD_T) push1(r, ls[v] * it, lt[v] * it);
    for (int v = sp.tail + tid; v < V1; v += KD_T) push1(r, ls[v] * it, lt[v] * it);
    // across the workgroup: the two maxima, then the sums rescaled to them (fixed trees: two runs are bit-equal)
    const float MA = block_max(r.mA, s_red), MB = block_max(r.mB, s_red);
    const float fB = __expf(r.mB - MB);
    const float SA = block_sum(r.sA * __expf(r.mA - MA), s_red);
    const float SB = block_sum(r.sB * fB, s_red);
    const float ACC = block_sum(r.acc * fB, s_red);
    if (tid != 0) return;
    const float lse_s = MA + logf(SA), lse_t = MB + logf(SB);
    a.lse_s[row] = lse_s;
    a.lse_t[row] = lse_t;
    a.kl[row] = ACC / SB - lse_t + lse_s;
    a.nll[row] = nll;
}

// the masked means of one launch's rows: double accumulators, a fixed order (deterministic).  The global sums take one row per
// thread (independent loads); the per-sample losses of per_row walk each sample's steps in order.
__global__ __launch_bounds__(FIN_T) void distill_finish_kernel(const KdArgs a) {
    __shared__ double s_red[4 * (FIN_T / 64)];
    const int tid = threadIdx.x;
    const int R = a.N * a.T;
    const double w_lm = 1.0 - (double)a.lambda, w_kd = (double)a.lambda * (double)a.tau * (double)a.tau;
    double s[4] = {0.0, 0.0, 0.0, 0.0};                      // mask, nll, kl, the mixed loss
    for (int row = tid; row < R; row += FIN_T) {
        const int i = row / a.T, t = row - i * a.T;
        const double m = a.mask[(size_t)i * a.mask_ld + t];
        if (m == 0.0) continue;
        const double nll = a.nll[row], kl = a.kl[row];
        s[0] += m;
        s[1] += m * nll;
        s[2] += m * kl;
        s[3] += m * (w_lm * nll + w_kd * kl);
    }
    if (a.per_row) {
        for (int i = tid; i < a.N; i += FIN_T) {
            double m_i = 0.0, c_i = 0.0;
            for (int t = 0; t < a.T; ++t) {
                const double m = a.mask[(size_t)i * a.mask_ld + t];
                if (m == 0.0) continue;
                const int row = i * a.T + t;
                m_i += m;
                c_i += m * (w_lm * (double)a.nll[row] + w_kd * (double)a.kl[row]);
            }
            a.loss_rows[i] = (float)c_i / (float)m_i;        // an all-zero row: 0 / 0 = NaN, as the other criteria
            a.msum[i] = (float)m_i;
        }
    }
    if (!fold_d<4, FIN_T>(s, s_red)) return;
    const float M = (float)s[0];
    a.out[0] = (float)s[1] / M;
    a.out[1] = (float)s[2] / M;
    a.out[2] = (float)s[3] / M;
    if (!a.per_row) a.msum[0] = M;
}

// d loss / d ls[row, v] = c (-(1 - lambda) [v == s] + lambda tau (pS_v - pT_v)),  c = u m / M
__global__ __launch_bounds__(KD_T) void distill_bwd_kernel(const KdArgs a) {
    const int row = blockIdx.x, tid = threadIdx.x;
    const int i = row / a.T, t = row - i * a.T;
    float *g = a.grad + (size_t)row * a.ld_grad;
    const float *ls = a.lp_s + (size_t)row * a.ld_s;
    const float *lt = a.lp_t + ((size_t)i * a.t_rows + t) * a.ld_t;
    const int V1 = a.V1;
    const float m = a.mask[(size_t)i * a.mask_ld + t];
    const bool soft = m != 0.f && a.lambda != 0.f;           // else the rows are not read
    const RowSplit sp = row_split(g, V1, !soft || (same16(g, ls) && same16(g, lt)));
    const int k = a.per_row ? i : 0;
    float ch = 0.f;
    int64_t s = -1;
    if (m != 0.f) {
        const float c = a.g_out[k] * m / a.msum[k];
        ch = -(1.f - a.lambda) * c;
        s = a.tok[(size_t)i * a.tok_ld + t];       // (a token outside [0, V1) matches no column: no hard-label term anywhere)
        if (soft) {
            const float ck = a.lambda * a.tau * c, it = a.inv_tau;
            const float lse_s = a.lse_s[row], lse_t = a.lse_t[row];
            const auto g1 = [&](float x, float y, int v) {
                return ck * (__expf(x * it - lse_s) - __expf(y * it - lse_t)) + (v == s ? ch : 0.f);
            };
            sweep<KD_T>(
                sp, tid,
                [&](int v0) {
                    const f32x4 x = ld4(ls + v0), y = ld4(lt + v0);
                    st4(g + v0, f32x4{g1(x.x, y.x, v0), g1(x.y, y.y, v0 + 1), g1(x.z, y.z, v0 + 2), g1(x.w, y.w, v0 + 3)});
                },
                [&](int v) { g[v] = g1(ls[v], lt[v], v); });
            return;
        }
    }
    sweep_one_hot<KD_T>(sp, tid, g, s, ch);                  // masked rows: zeros; lambda == 0: the hard-label term alone
}

int common_args(const capmi_distill *p, KdArgs &a) {
    if (!p || p->N < 0 || p->T < 1 || p->V1 < 1) return CAPMI_EINVAL;
    if (p->ld_s < p->V1 || p->ld_t < p->V1 || p->t_rows < p->T || p->tok_ld < p->T || p->mask_ld < p->T) return CAPMI_EINVAL;
    if ((int64_t)p->N * p->T > 0x7fffffff) return CAPMI_EINVAL;
    if (!(p->tau > 0.f) || p->tau == INFINITY) return CAPMI_EINVAL;
    if (!(p->lambda >= 0.f && p->lambda <= 1.f)) return CAPMI_EINVAL;
    if (!p->lp_s || !p->lp_t || !p->tok || !p->mask || !p->row_stats || !p->msum) return CAPMI_EINVAL;
    if (!aligned4(p->lp_s, p->lp_t, p->mask, p->row_stats, p->msum)) return CAPMI_EINVAL;
    a = KdArgs{};
    a.lp_s = p->lp_s, a.lp_t = p->lp_t, a.tok = p->tok, a.mask = p->mask;
    const size_t R = (size_t)p->N * p->T;
    a.lse_s = p->row_stats, a.lse_t = p->row_stats + R, a.kl = p->row_stats + 2 * R, a.nll = p->row_stats + 3 * R;
    a.msum = p->msum, a.out = p->out, a.loss_rows = p->loss_rows, a.g_out = p->g_out, a.grad = p->grad;
    a.N = p->N, a.T = p->T, a.V1 = p->V1, a.ld_s = p->ld_s, a.ld_t = p->ld_t, a.ld_grad = p->ld_grad, a.t_rows = p->t_rows;
    a.tok_ld = p->tok_ld, a.mask_ld = p->mask_ld;
    a.per_row = p->per_row ? 1 : 0;
    a.lambda = p->lambda, a.tau = p->tau, a.inv_tau = 1.f / p->tau;
    return 0;
}

}  // namespace

extern "C" int capmi_distill_loss_fwd(const capmi_distill *p, void *stream) {
    KdArgs a;
    if (common_args(p, a) != 0) return CAPMI_EINVAL;
    if (!p->out || (p->per_row && !p->loss_rows)) return CAPMI_EINVAL;
    if (p->N == 0) return 0;
    const int R = p->N * p->T;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(distill_rows_kernel, dim3(R), dim3(KD_T), 0, st, a);
    CAPMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(FIN_T), 0, st, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_distill_loss_bwd(const capmi_distill *p, void *stream) {
    KdArgs a;
    if (common_args(p, a) != 0) return CAPMI_EINVAL;
    if (p->ld_grad < p->V1 || !p->grad || !p->g_out || !aligned4(p->grad, p->g_out)) return CAPMI_EINVAL;
    if (p->N == 0) return 0;
    hipLaunchKernelGGL(distill_bwd_kernel, dim3(p->N * p->T), dim3(KD_T), 0, (hipStream_t)stream, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
