// BatchNorm1d over the valid region rows (use_bn: AttModel.py:80-85 under pack_wrapper, :44-49): statistics, apply, backward.
//
// X is [rows, D] fp32 (rows = B * K), `mask` one float per row (0 = padded region, NULL = every row valid).  The statistics are taken
// over the M valid rows; M is counted on the device and never read by the host.
//
// Bottom-up features are post-ReLU: columns are non-negative, often exactly zero, and can have mean >> std, so the one-pass
// E[x^2] - E[x]^2 form is not used.  Instead (Chan, Golub & LeVeque 1983):
//   bn_stats_kernel     one wave per (16 rows x 256 columns) tile, a thread owns 4 adjacent columns.  Every value is first shifted by
//                       the column's PIVOT, its value in the first valid row: a column with mean 100 and std 0.01 keeps the digits of
//                       its deviations, which a block mean stored as one float near 100 (ulp 7.6e-6) would lose -- the spread of the
//                       block means, 0.0025 here, is what the merge below squares.  The tile's 16 shifted values of a column stay in
//                       registers: n = valid rows, mean_b = sum / n, M2_b = sum (v - mean_b)^2, rows in order.  One read of X.
//   bn_finalize_kernel  a thread per column merges the row blocks IN BLOCK ORDER: delta = mean_b - mean; mean += delta * n_b / n';
//                       M2 += M2_b + delta^2 * n * n_b / n'.  Then mean += pivot, rstd = 1 / sqrt(M2 / M + eps) and, in place and on the stream,
//                       running_mean / running_var (unbiased, M / (M - 1)) with the momentum, and num_batches_tracked += 1.
// No atomics, a fixed tree: two calls on the same input give the same bits.  M < 2 (torch raises there; checking would need the host
// to wait): the batch statistics are those of the M rows (mean 0 / the row, variance 0), the running buffers and the counter are left
// untouched -- nothing is divided by M - 1, no NaN reaches them.
//
// A row of D floats is in general not 16-byte aligned (D = 2053: 2053 * 4 = 4 mod 16, and the misalignment changes from row to row),
// and a thread must keep its columns over all rows of its tile.  So the 16-byte path is taken per launch, where D % 4 == 0 and the
// bases are 16-byte aligned -- every row then is --, and the dword path otherwise: the 4 dword loads of a wave still cover one
// contiguous 1 KiB per row.
//
//   bn_apply_kernel       y = ((x - pivot) - (mean - pivot)) * rstd * gamma + beta on valid rows, 0 on padded ones: the mean travels as
//                         the pair `shift` the finalize wrote.  Rounded to one float, a mean near 100 is off by up to 3.8e-6, which a
//                         column of std 0.01 would see as 4e-4 in its normalised values.  (Eval: pivot 0, offset running_mean.)
//   bn_bwd_partial_kernel per row block sum dy and sum dy * xhat over the valid rows (the same tiles as the statistics)
//   bn_colsum_parts       sums such per-block partials in block order (d gamma, d beta)
//   bn_bwd_dx_kernel      dx = gamma * rstd * (dy - (d beta + xhat * d gamma) / M) on valid rows (train), gamma * rstd * dy (eval), 0 on
//                         padded ones
//   bn_linear_bwd_kernel  BN in FRONT of a Linear whose input needs no gradient: with G0 = d_pre^T X on the raw input and db = colsum d_pre,
//                         G = (G0 - db mean^T) diag(rstd), dW = G diag(gamma) + db beta^T, d gamma_j = sum_r W_rj G_rj, d beta_j = sum_r W_rj db_r
//                         -- an [R, D] pass instead of an [M, D] dX product; partials per 16 rows of W, summed by bn_colsum_parts.
#include "host_common.h"

using namespace capmi;

namespace {

constexpr int ROWS = 16;                 // rows of a tile
constexpr int COLS = 4 * CAPMI_WAVE;     // columns of a tile: 4 per lane

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float *row, int c, int D) {
    if (VEC) return *reinterpret_cast<const f32x4 *>(row + c);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c + e < D) v[e] = row[c + e];
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float *row, int c, int D, f32x4 v) {
    if (VEC) {
        *reinterpret_cast<f32x4 *>(row + c) = v;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c + e < D) row[c + e] = v[e];
}

// the first valid row (0 when there is none): its values are the pivot every block subtracts.  Masks are prefix masks, so this is
// row 0 unless the first image has no region at all; the scan is the same in every thread.
__device__ __forceinline__ int pivot_row(const float *mask, int rows) {
    int p = 0;
    if (mask) {
        while (p < rows && mask[p] == 0.f) ++p;
        if (p == rows) p = 0;
    }
    return p;
}

// partial: [nrb][2][D] (mean_b - pivot, M2_b), then [nrb] valid-row counts
template <bool VEC>
__global__ __launch_bounds__(CAPMI_WAVE) void bn_stats_kernel(const float *__restrict__ x, const float *__restrict__ mask, int rows,
                                                              int D, int nrb, float *__restrict__ partial) {
    const int c = blockIdx.x * COLS + 4 * threadIdx.x;
    const int rb = blockIdx.y, r0 = rb * ROWS;
    unsigned valid = 0;
    int n = 0;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int r = r0 + i;
        if (r < rows && (!mask || mask[r] != 0.f)) { valid |= 1u << i; ++n; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) partial[(size_t)nrb * 2 * D + rb] = (float)n;
    if (c >= D) return;
    const f32x4 piv = load4<VEC>(x + (size_t)pivot_row(mask, rows) * D, c, D);
    f32x4 v[ROWS];
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid >> i & 1) {
            v[i] = load4<VEC>(x + (size_t)(r0 + i) * D, c, D) - piv;
            s += v[i];
        }
    }
    const float inv = n > 0 ? 1.f / (float)n : 0.f;
    const f32x4 mean = s * inv;
    f32x4 m2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        if (valid >> i & 1) {
            const f32x4 d = v[i] - mean;
            m2 += d * d;
        }
    }
    store4<VEC>(partial + (size_t)(rb * 2 + 0) * D, c, D, mean);
    store4<VEC>(partial + (size_t)(rb * 2 + 1) * D, c, D, m2);
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const float *__restrict__ partial, const float *__restrict__ x,
                                                          const float *__restrict__ mask, int rows, int D, int nrb, int train, float eps,
                                                          float momentum, float *__restrict__ running_mean,
                                                          float *__restrict__ running_var, int64_t *__restrict__ nbt,
                                                          float *__restrict__ mean_out, float *__restrict__ rstd_out,
                                                          float *__restrict__ count_out, float *__restrict__ shift) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (!train) {
        if (j < D) {
            shift[j] = 0.f;
            shift[D + j] = running_mean[j];
            mean_out[j] = running_mean[j];
            rstd_out[j] = 1.f / sqrtf(running_var[j] + eps);
        }
        if (j == 0 && count_out) count_out[0] = 0.f;
        return;
    }
    const float *counts = partial + (size_t)nrb * 2 * D;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    if (j < D) {
        for (int rb = 0; rb < nrb; ++rb) {
            const float nb = counts[rb];
            if (nb == 0.f) continue;
            const float mb = partial[(size_t)(rb * 2 + 0) * D + j], m2b = partial[(size_t)(rb * 2 + 1) * D + j];
            const float nn = n + nb, delta = mb - mean;
            mean += delta * (nb / nn);
            m2 += m2b + delta * delta * (n * nb / nn);
            n = nn;
        }
    }
    if (j == 0) {
        if (count_out) count_out[0] = n;
        if (nbt && n >= 2.f) nbt[0] += 1;
    }
    if (j >= D) return;
    const float var = n > 0.f ? m2 / n : 0.f;
    const float piv = n > 0.f ? x[(size_t)pivot_row(mask, rows) * D + j] : 0.f;
    shift[j] = piv;                 // the mean as (pivot, offset): bn_apply subtracts both and keeps the digits their sum rounds away
    shift[D + j] = mean;
    mean = piv + mean;
    mean_out[j] = mean;
    rstd_out[j] = 1.f / sqrtf(var + eps);
    if (n >= 2.f && running_mean && running_var) {
        running_mean[j] = (1.f - momentum) * running_mean[j] + momentum * mean;
        running_var[j] = (1.f - momentum) * running_var[j] + momentum * (m2 / (n - 1.f));
    }
}

// x / y (and dy / dx below) carry no __restrict__: the output may be the input (capmi.h)
template <bool VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float *x, const float *__restrict__ mask,
                                                       const float *__restrict__ shift, const float *__restrict__ rstd,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       float *y, int rows, int D) {
    const int qd = (D + 3) / 4;
    const size_t total = (size_t)rows * qd;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(q / qd), c = (int)(q % qd) * 4;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (!mask || mask[r] != 0.f) {
            const f32x4 v = load4<VEC>(x + (size_t)r * D, c, D);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < D) o[e] = ((v[e] - shift[c + e]) - shift[D + c + e]) * rstd[c + e] * gamma[c + e] + beta[c + e];
        }
        store4<VEC>(y + (size_t)r * D, c, D, o);
    }
}

// partial: [nrb][2][D] (sum dy, sum dy * xhat)
template <bool VEC>
__global__ __launch_bounds__(CAPMI_WAVE) void bn_bwd_partial_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                                    const float *__restrict__ mask, const float *__restrict__ mean,
                                                                    const float *__restrict__ rstd, int rows, int D,
                                                                    float *__restrict__ partial) {
    const int c = blockIdx.x * COLS + 4 * threadIdx.x;
    if (c >= D) return;
    const int rb = blockIdx.y, r0 = rb * ROWS;
    f32x4 mu, rs;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mu[e] = c + e < D ? mean[c + e] : 0.f;
        rs[e] = c + e < D ? rstd[c + e] : 0.f;
    }
    f32x4 sb = {0.f, 0.f, 0.f, 0.f}, sg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = 0; i < ROWS; ++i) {
        const int r = r0 + i;
        if (r < rows && (!mask || mask[r] != 0.f)) {
            const f32x4 g = load4<VEC>(dy + (size_t)r * D, c, D);
            const f32x4 v = load4<VEC>(x + (size_t)r * D, c, D);
            sb += g;
            sg += g * ((v - mu) * rs);
        }
    }
    store4<VEC>(partial + (size_t)(rb * 2 + 0) * D, c, D, sb);
    store4<VEC>(partial + (size_t)(rb * 2 + 1) * D, c, D, sg);
}

__global__ __launch_bounds__(256) void bn_colsum_parts_kernel(const float *__restrict__ partial, int nparts, int D,
                                                              float *__restrict__ out0, float *__restrict__ out1) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= D) return;
    float a = 0.f, b = 0.f;
    for (int p = 0; p < nparts; ++p) {
        a += partial[(size_t)(p * 2 + 0) * D + j];
        b += partial[(size_t)(p * 2 + 1) * D + j];
    }
    if (out0) out0[j] = a;
    if (out1) out1[j] = b;
}

template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const float *dy, const float *__restrict__ x,
                                                        const float *__restrict__ mask, const float *__restrict__ mean,
                                                        const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                        const float *__restrict__ dgamma, const float *__restrict__ dbeta,
                                                        const float *__restrict__ count, int train, float *dx, int rows,
                                                        int D) {
    const int qd = (D + 3) / 4;
    const size_t total = (size_t)rows * qd;
    float invM = 0.f;
    if (train) {
        const float M = count[0];
        invM = M > 0.f ? 1.f / M : 0.f;
    }
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(q / qd), c = (int)(q % qd) * 4;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (!mask || mask[r] != 0.f) {
            const f32x4 g = load4<VEC>(dy + (size_t)r * D, c, D);
            const f32x4 v = load4<VEC>(x + (size_t)r * D, c, D);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e >= D) continue;
                const float a = gamma[c + e] * rstd[c + e];
                if (train) {
                    const float xh = (v[e] - mean[c + e]) * rstd[c + e];
                    o[e] = a * (g[e] - (dbeta[c + e] + xh * dgamma[c + e]) * invM);
                } else {
                    o[e] = a * g[e];
                }
            }
        }
        store4<VEC>(dx + (size_t)r * D, c, D, o);
    }
}

// G (in: G0 = d_pre^T X, out: dW) [R][D]; partial [ceil(R / ROWS)][2][D] (sum_r W G, sum_r W db)
template <bool VEC>
__global__ __launch_bounds__(CAPMI_WAVE) void bn_linear_bwd_kernel(float *__restrict__ G, const float *__restrict__ db,
                                                                   const float *__restrict__ W, const float *__restrict__ mean,
                                                                   const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta, int R, int D,
                                                                   float *__restrict__ partial) {
    const int c = blockIdx.x * COLS + 4 * threadIdx.x;
    if (c >= D) return;
    const int rb = blockIdx.y, r0 = rb * ROWS;
    f32x4 mu, rs, ga, be;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool in = c + e < D;
        mu[e] = in ? mean[c + e] : 0.f;
        rs[e] = in ? rstd[c + e] : 0.f;
        ga[e] = in ? gamma[c + e] : 0.f;
        be[e] = in ? beta[c + e] : 0.f;
    }
    f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = 0; i < ROWS; ++i) {
        const int r = r0 + i;
        if (r >= R) break;
        const float d = db[r];
        const f32x4 g0 = load4<VEC>(G + (size_t)r * D, c, D);
        const f32x4 w = load4<VEC>(W + (size_t)r * D, c, D);
        const f32x4 g = (g0 - mu * d) * rs;
        sg += w * g;
        sb += w * d;
        store4<VEC>(G + (size_t)r * D, c, D, g * ga + be * d);
    }
    store4<VEC>(partial + (size_t)(rb * 2 + 0) * D, c, D, sg);
    store4<VEC>(partial + (size_t)(rb * 2 + 1) * D, c, D, sb);
}

inline bool vec_ok(int D) { return D % 4 == 0; }
inline bool bad4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }
inline dim3 tile_grid(int rows, int D) { return dim3((D + COLS - 1) / COLS, (rows + ROWS - 1) / ROWS); }

}  // namespace

extern "C" {

int capmi_bn_row_blocks(int rows) { return rows > 0 ? (rows + ROWS - 1) / ROWS : 0; }

int capmi_bn_stats(const float *x, const float *mask, int rows, int D, float *partial, void *stream) {
    if (!x || !partial || rows <= 0 || D <= 0 || bad4(x) || bad4(mask) || bad4(partial)) return CAPMI_EINVAL;
    const int nrb = capmi_bn_row_blocks(rows);
    if (nrb > 65535) return CAPMI_EINVAL;
    if (vec_ok(D) && aligned16(x, partial))
        hipLaunchKernelGGL(bn_stats_kernel<true>, tile_grid(rows, D), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, x, mask, rows, D, nrb,
                           partial);
    else
        hipLaunchKernelGGL(bn_stats_kernel<false>, tile_grid(rows, D), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, x, mask, rows, D, nrb,
                           partial);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_bn_finalize(const float *partial, const float *x, const float *mask, int rows, int D, int train, float eps, float momentum,
                      float *running_mean, float *running_var, int64_t *num_batches_tracked, float *mean, float *rstd, float *count,
                      float *shift, void *stream) {
    if (D <= 0 || !mean || !rstd || !shift || bad4(shift) || bad4(mean) || bad4(rstd) || bad4(running_mean) || bad4(running_var) || bad4(count) ||
        bad4(partial) || bad4(x) || bad4(mask))
        return CAPMI_EINVAL;
    if (train && (!partial || !x || rows <= 0)) return CAPMI_EINVAL;
    if (!train && (!running_mean || !running_var)) return CAPMI_EINVAL;
    if (reinterpret_cast<uintptr_t>(num_batches_tracked) & 7) return CAPMI_EINVAL;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, partial, x, mask, rows, D,
                       train ? capmi_bn_row_blocks(rows) : 0, train, eps, momentum, running_mean, running_var, num_batches_tracked, mean,
                       rstd, count, shift);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_bn_apply(const float *x, const float *mask, const float *shift, const float *rstd, const float *gamma, const float *beta,
                   float *y, int rows, int D, void *stream) {
    if (!x || !shift || !rstd || !gamma || !beta || !y || rows <= 0 || D <= 0 || bad4(x) || bad4(y) || bad4(mask) || bad4(shift) ||
        bad4(rstd) || bad4(gamma) || bad4(beta))
        return CAPMI_EINVAL;
    const size_t quads = (size_t)rows * ((D + 3) / 4);
    if (vec_ok(D) && aligned16(x, y))
        hipLaunchKernelGGL(bn_apply_kernel<true>, dim3(grid_for(quads)), dim3(256), 0, (hipStream_t)stream, x, mask, shift, rstd, gamma,
                           beta, y, rows, D);
    else
        hipLaunchKernelGGL(bn_apply_kernel<false>, dim3(grid_for(quads)), dim3(256), 0, (hipStream_t)stream, x, mask, shift, rstd, gamma,
                           beta, y, rows, D);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_bn_bwd_partial(const float *dy, const float *x, const float *mask, const float *mean, const float *rstd, int rows, int D,
                         float *partial, void *stream) {
    if (!dy || !x || !mean || !rstd || !partial || rows <= 0 || D <= 0 || bad4(dy) || bad4(x) || bad4(mask) || bad4(partial) ||
        bad4(mean) || bad4(rstd))
        return CAPMI_EINVAL;
    if (capmi_bn_row_blocks(rows) > 65535) return CAPMI_EINVAL;
    if (vec_ok(D) && aligned16(dy, x, partial))
        hipLaunchKernelGGL(bn_bwd_partial_kernel<true>, tile_grid(rows, D), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, dy, x, mask, mean,
                           rstd, rows, D, partial);
    else
        hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, tile_grid(rows, D), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, dy, x, mask, mean,
                           rstd, rows, D, partial);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_bn_colsum_parts(const float *partial, int nparts, int D, float *out0, float *out1, void *stream) {
    if (!partial || nparts <= 0 || D <= 0 || bad4(partial) || bad4(out0) || bad4(out1)) return CAPMI_EINVAL;
    hipLaunchKernelGGL(bn_colsum_parts_kernel, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, partial, nparts, D, out0, out1);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_bn_bwd_dx(const float *dy, const float *x, const float *mask, const float *mean, const float *rstd, const float *gamma,
                    const float *dgamma, const float *dbeta, const float *count, int train, float *dx, int rows, int D, void *stream) {
    if (!dy || !x || !mean || !rstd || !gamma || !dx || rows <= 0 || D <= 0 || bad4(dy) || bad4(x) || bad4(dx) || bad4(mask) ||
        bad4(mean) || bad4(rstd) || bad4(gamma) || bad4(dgamma) || bad4(dbeta) || bad4(count))
        return CAPMI_EINVAL;
    if (train && (!dgamma || !dbeta || !count)) return CAPMI_EINVAL;
    const size_t quads = (size_t)rows * ((D + 3) / 4);
    if (vec_ok(D) && aligned16(dy, x, dx))
        hipLaunchKernelGGL(bn_bwd_dx_kernel<true>, dim3(grid_for(quads)), dim3(256), 0, (hipStream_t)stream, dy, x, mask, mean, rstd,
                           gamma, dgamma, dbeta, count, train, dx, rows, D);
    else
        hipLaunchKernelGGL(bn_bwd_dx_kernel<false>, dim3(grid_for(quads)), dim3(256), 0, (hipStream_t)stream, dy, x, mask, mean, rstd,
                           gamma, dgamma, dbeta, count, train, dx, rows, D);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_bn_linear_bwd(float *G, const float *db, const float *W, const float *mean, const float *rstd, const float *gamma,
                        const float *beta, int R, int D, float *partial, void *stream) {
    if (!G || !db || !W || !mean || !rstd || !gamma || !beta || !partial || R <= 0 || D <= 0 || bad4(G) || bad4(W) || bad4(partial) ||
        bad4(db) || bad4(mean) || bad4(rstd) || bad4(gamma) || bad4(beta))
        return CAPMI_EINVAL;
    if (capmi_bn_row_blocks(R) > 65535) return CAPMI_EINVAL;
    if (vec_ok(D) && aligned16(G, W, partial))
        hipLaunchKernelGGL(bn_linear_bwd_kernel<true>, tile_grid(R, D), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, G, db, W, mean, rstd,
                           gamma, beta, R, D, partial);
    else
        hipLaunchKernelGGL(bn_linear_bwd_kernel<false>, tile_grid(R, D), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, G, db, W, mean, rstd,
                           gamma, beta, R, D, partial);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
