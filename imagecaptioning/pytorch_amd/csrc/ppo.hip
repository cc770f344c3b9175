// PPO structure loss (gfx950): clipped policy ratio + KL(old || new) of the sampled rollout against a frozen old policy.
// Reference: PPOLoss.forward (captioning/modules/losses.py:267-357).  See include/capmi.h (capmi_ppo_loss_fwd / _bwd) for the
// contract and the edge cases.  Forward: one workgroup per (n, t) row reads the new and the old row once, then one workgroup folds
// the masked means.  Backward: one workgroup per row reads the old row once and writes the dense gradient once.  Rows are cut and
// swept, and the means folded, as row_sweep.h has it.
#include "host_common.h"
#include "row_sweep.h"

using namespace capmi;

namespace {

constexpr int PPO_T = 256;             // 4 waves per row: 9.3 float4 per thread at V1 = 9488
constexpr int PPO_W = PPO_T / 64;
constexpr int FIN_T = 1024;

struct PpoArgs {
    const float *lp_new, *lp_old;
    const int64_t *seq;
    const float *scores;
    float *kl, *r, *pg, *gpg;          // the four planes of row_stats
    float *msum, *out, *loss_rows;
    const float *g_out;
    float *grad;
    int N, L, V1, n, ld_new, ld_old, ld_grad, per_row;
    float eps, kl_coef;
    int vec;                           // new and old rows share one alignment mod 16 bytes: float4 body
};

// mask of row (i, t): position 0 always counts, later ones while the previous token was not the end token
__device__ __forceinline__ bool row_on(const int64_t *seq, int L, int i, int t) { return t == 0 || seq[(size_t)i * L + t - 1] > 0; }

// exp(lo) * (lo - ln): F.kl_div(ln, lo, log_target=True) elementwise, IEEE cases included (lo = -inf gives NaN as there)
__device__ __forceinline__ float kl1(float lo, float ln) { return __expf(lo) * (lo - ln); }

// torch.maximum: NaN if either side is NaN
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b); }

__global__ __launch_bounds__(PPO_T) void ppo_rows_kernel(const PpoArgs a) {
    __shared__ float s_red[PPO_W];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int i = row / a.L, t = row - i * a.L;
    if (!row_on(a.seq, a.L, i, t)) {                         // masked: nothing read (capmi.h)
        if (tid == 0) a.kl[row] = 0.f, a.r[row] = 0.f, a.pg[row] = 0.f, a.gpg[row] = 0.f;
        return;
    }
    const float *ln = a.lp_new + (size_t)row * a.ld_new;
    const float *lo = a.lp_old + (size_t)row * a.ld_old;
    const int V1 = a.V1;
    const RowSplit sp = row_split(ln, V1, a.vec);
    // the sampled token's two entries and the image's scores: loaded before the sweep, so their latency hides behind it
    const int64_t s = a.seq[(size_t)i * a.L + t];
    const bool s_in = s >= 0 && s < V1;
    float ln_s = 0.f, lo_s = 0.f, tot = 0.f, si = 0.f;
    const int img = i / a.n;
    if (tid == 0) {
        if (s_in) ln_s = ln[s], lo_s = lo[s];
        for (int k = 0; k < a.n; ++k) tot += a.scores[img * a.n + k];
        si = a.scores[i];
    }
    float acc = 0.f;
    sweep<PPO_T>(
        sp, tid,
        [&](int v0) {
            const f32x4 x = ld4(ln + v0), y = ld4(lo + v0);
            acc += (kl1(y.x, x.x) + kl1(y.y, x.y)) + (kl1(y.z, x.z) + kl1(y.w, x.w));
        },
        [&](int v) { acc += kl1(lo[v], ln[v]); });
    const float kl = block_sum(acc, s_red);
    if (tid != 0) return;
    // the advantage of sample i against the mean score of its image's other samples (new_self_critical's baseline)
    const float A = si - (tot - si) / (float)(a.n - 1);
    const float r = s_in ? expf(ln_s - lo_s) : __builtin_nanf("");    // (a token outside the row: NaN, no read)
    const float lo_c = 1.f - a.eps, hi_c = 1.f + a.eps;
    const float p1 = -A * r, p2 = -A * fminf(fmaxf(r, lo_c), hi_c);
    const float pg = nan_max(p1, p2);
    // d pg / d ln_s, torch.maximum's backward (a tie splits the gradient) times exp's and clamp's; a side that does not get
    // the gradient contributes nothing, also where its value is infinite (capmi.h)
    const float in_clip = (r >= lo_c && r <= hi_c) ? 1.f : 0.f;
    float g;
    if (p1 > p2) g = -A * r;
    else if (p2 > p1) g = in_clip != 0.f ? -A * r : 0.f;
    else if (p1 == p2) g = in_clip != 0.f ? -A * r : 0.5f * (-A * r);
    else g = __builtin_nanf("");
    a.kl[row] = kl;
    a.r[row] = r;
    a.pg[row] = pg;
    a.gpg[row] = g;
}

// the masked means of one launch's rows: double accumulators, a fixed order (deterministic).  The global sums take one row per
// thread (independent loads); the per-sample losses of per_row walk each sample's steps in order.
__global__ __launch_bounds__(FIN_T) void ppo_finish_kernel(const PpoArgs a) {
    __shared__ double s_red[4 * (FIN_T / 64)];
    const int tid = threadIdx.x;
    const int R = a.N * a.L;
    double s[4] = {0.0, 0.0, 0.0, 0.0};                      // rows on, pg, kl, clipped
    for (int row = tid; row < R; row += FIN_T) {
        const int i = row / a.L, t = row - i * a.L;
        if (!row_on(a.seq, a.L, i, t)) continue;
        s[0] += 1.0;
        s[1] += a.pg[row];
        s[2] += a.kl[row];
        s[3] += fabsf(a.r[row] - 1.f) > a.eps ? 1.0 : 0.0;
    }
    if (a.per_row) {
        for (int i = tid; i < a.N; i += FIN_T) {
            float m_i = 0.f, loss_i = 0.f;
            for (int t = 0; t < a.L; ++t) {
                if (!row_on(a.seq, a.L, i, t)) continue;
                const int row = i * a.L + t;
                m_i += 1.f;
                loss_i += a.pg[row] + a.kl_coef * a.kl[row];
            }
            a.loss_rows[i] = loss_i / m_i;
            a.msum[i] = m_i;
        }
    }
    if (!fold_d<4, FIN_T>(s, s_red)) return;
    const float M = (float)s[0];
    const float pg_loss = (float)s[1] / M, kl_loss = (float)s[2] / M;
    a.out[0] = pg_loss;
    a.out[1] = kl_loss;
    a.out[2] = (float)s[3] / M;
    a.out[3] = pg_loss + a.kl_coef * kl_loss;
    if (!a.per_row) a.msum[0] = M;
}

// d loss / d ln[row, v] = c * (-kl_coef * exp(lo[row, v]) + [v == s] * g_pg[row]),  c = u * m / M
__global__ __launch_bounds__(PPO_T) void ppo_bwd_kernel(const PpoArgs a) {
    const int row = blockIdx.x, tid = threadIdx.x;
    const int i = row / a.L, t = row - i * a.L;
    float *g = a.grad + (size_t)row * a.ld_grad;
    const int V1 = a.V1;
    const bool on = row_on(a.seq, a.L, i, t);
    const RowSplit sp = row_split(g, V1, a.vec);
    if (!on) {                                               // masked rows: zeros, the old row is not read
        sweep_one_hot<PPO_T>(sp, tid, g, -1, 0.f);
        return;
    }
    const float c = a.per_row ? a.g_out[i] / a.msum[i] : a.g_out[0] / a.msum[0];
    const float ck = -a.kl_coef * c;
    const float cs = c * a.gpg[row];
    const int64_t s = a.seq[(size_t)i * a.L + t];   // (a token outside [0, V1) matches no column: no extra term anywhere)
    const float *lo = a.lp_old + (size_t)row * a.ld_old;
    const auto g1 = [&](float y, int v) { return ck * __expf(y) + (v == s ? cs : 0.f); };
    sweep<PPO_T>(
        sp, tid,
        [&](int v0) {
            const f32x4 y = ld4(lo + v0);
            st4(g + v0, f32x4{g1(y.x, v0), g1(y.y, v0 + 1), g1(y.z, v0 + 2), g1(y.w, v0 + 3)});
        },
        [&](int v) { g[v] = g1(lo[v], v); });
}

int common_args(const capmi_ppo *p, PpoArgs &a) {
    if (!p || p->N < 0 || p->L < 1 || p->V1 < 1 || p->n < 2 || (p->N % p->n) != 0 || p->ld_old < p->V1 || !p->lp_old || !p->seq)
        return CAPMI_EINVAL;
    if ((int64_t)p->N * p->L > 0x7fffffff) return CAPMI_EINVAL;
    if (!aligned4(p->lp_old)) return CAPMI_EINVAL;
    if (!(p->eps >= 0.f) || !(p->kl_coef >= 0.f) || p->eps == INFINITY || p->kl_coef == INFINITY) return CAPMI_EINVAL;
    a = PpoArgs{};
    a.lp_new = p->lp_new, a.lp_old = p->lp_old, a.seq = p->seq, a.scores = p->scores;
    const size_t R = (size_t)p->N * p->L;
    if (p->row_stats) a.kl = p->row_stats, a.r = p->row_stats + R, a.pg = p->row_stats + 2 * R, a.gpg = p->row_stats + 3 * R;
    a.msum = p->msum, a.out = p->out, a.loss_rows = p->loss_rows, a.g_out = p->g_out, a.grad = p->grad;
    a.N = p->N, a.L = p->L, a.V1 = p->V1, a.n = p->n, a.ld_new = p->ld_new, a.ld_old = p->ld_old, a.ld_grad = p->ld_grad;
    a.per_row = p->per_row ? 1 : 0;
    a.eps = p->eps, a.kl_coef = p->kl_coef;
    return 0;
}

}  // namespace

extern "C" int capmi_ppo_loss_fwd(const capmi_ppo *p, void *stream) {
    PpoArgs a;
    if (common_args(p, a) != 0) return CAPMI_EINVAL;
    if (p->ld_new < p->V1 || !p->lp_new || !p->scores || !p->row_stats || !p->msum || !p->out || (p->per_row && !p->loss_rows))
        return CAPMI_EINVAL;
    if (!aligned4(p->lp_new)) return CAPMI_EINVAL;
    const int R = p->N * p->L;
    if (overlaps(p->row_stats, (size_t)4 * R * sizeof(float), p->lp_new, span(R, p->ld_new, p->V1)) ||
        overlaps(p->row_stats, (size_t)4 * R * sizeof(float), p->lp_old, span(R, p->ld_old, p->V1)))
        return CAPMI_EINVAL;
    a.vec = same_phase16(p->lp_new, p->ld_new, p->lp_old, p->ld_old) ? 1 : 0;
    if (p->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppo_rows_kernel, dim3(R), dim3(PPO_T), 0, st, a);
    CAPMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(ppo_finish_kernel, dim3(1), dim3(FIN_T), 0, st, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_ppo_loss_bwd(const capmi_ppo *p, void *stream) {
    PpoArgs a;
    if (common_args(p, a) != 0) return CAPMI_EINVAL;
    if (p->ld_grad < p->V1 || !p->grad || !p->row_stats || !p->msum || !p->g_out) return CAPMI_EINVAL;
    if (!aligned4(p->grad)) return CAPMI_EINVAL;
    const int R = p->N * p->L;
    if (overlaps(p->grad, span(R, p->ld_grad, p->V1), p->lp_old, span(R, p->ld_old, p->V1))) return CAPMI_EINVAL;
    a.vec = same_phase16(p->grad, p->ld_grad, p->lp_old, p->ld_old) ? 1 : 0;
    if (p->N == 0) return 0;
    hipLaunchKernelGGL(ppo_bwd_kernel, dim3(R), dim3(PPO_T), 0, (hipStream_t)stream, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
