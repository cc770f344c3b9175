// The att2ctx stage of an AoA decode step for the decoder types of the ablation table (AoAModel.py:141-149, 172-185) on gfx950:
// siblings of glu_fwd_fused_kernel (transformer.hip) that consume the same K-slice slab layout and write the same outputs and
// bf16x3 planes.  HBM / latency bound pointwise work: 16-byte accesses, 4 columns per thread, every slab load of a trip issued
// before the first is consumed.
#include "host_common.h"
#include "profile.h"

using namespace capmi;

namespace {

// G column blocks of R per row: 1 = Linear -> ReLU ("base"), 2 = Linear -> GLU (AoA), 4 = LSTMCell gates (i, f, g, o).
// Slabs are summed in order from 0.f, 4 per trip, then the biases: the order of glu_fwd_fused_kernel (G = 2 gives its bits).
template <int G>
__global__ __launch_bounds__(256) void ctx_fwd_fused_kernel(const capmi_ctx_step s) {
    const int R = s.R, q4 = R >> 2;
    const size_t nq = (size_t)s.M * q4;
    unsigned char *pl_a = static_cast<unsigned char *>(s.planes_a), *pl_b = static_cast<unsigned char *>(s.planes_b);
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(q / q4), c = (int)(q % q4) * 4;
        const size_t ip = (size_t)r * G * R + c, io = (size_t)r * R + c;
        f32x4 acc[G];
#pragma unroll
        for (int k = 0; k < G; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < s.splits; s0 += 4) {
            f32x4 tv[4][G];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t o = (size_t)min(s0 + u, s.splits - 1) * (size_t)s.stride;
#pragma unroll
                for (int k = 0; k < G; ++k) tv[u][k] = *reinterpret_cast<const f32x4 *>(s.slabs + o + ip + (size_t)k * R);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (s0 + u < s.splits) {
#pragma unroll
                    for (int k = 0; k < G; ++k) acc[k] += tv[u][k];
                }
        }
#pragma unroll
        for (int k = 0; k < G; ++k) {
            if (s.bias) acc[k] += *reinterpret_cast<const f32x4 *>(s.bias + (size_t)k * R + c);
            if (s.bias2) acc[k] += *reinterpret_cast<const f32x4 *>(s.bias2 + (size_t)k * R + c);
        }
        f32x4 o;
        if (G == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaxf(acc[0][e], 0.f);
        } else if (G == 2) {
#pragma unroll
            for (int k = 0; k < G; ++k) *reinterpret_cast<f32x4 *>(s.pre + ip + (size_t)k * R) = acc[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = acc[0][e] * sigmoid_f(acc[G > 1 ? 1 : 0][e]);
        } else {
            const f32x4 cp = *reinterpret_cast<const f32x4 *>(s.c_prev + io);
            f32x4 cn;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ig = sigmoid_f(acc[0][e]), fg = sigmoid_f(acc[G > 1 ? 1 : 0][e]);
                const float gg = tanh_f(acc[G > 2 ? 2 : 0][e]), og = sigmoid_f(acc[G > 3 ? 3 : 0][e]);
                acc[0][e] = ig; acc[G > 1 ? 1 : 0][e] = fg; acc[G > 2 ? 2 : 0][e] = gg; acc[G > 3 ? 3 : 0][e] = og;
                cn[e] = fg * cp[e] + ig * gg;
                o[e] = og * tanh_f(cn[e]);
            }
            *reinterpret_cast<f32x4 *>(s.c + io) = cn;
            if (s.pre) {                               // the activated gates, the layout capmi_lstm_cell_bwd_partial reads
#pragma unroll
                for (int k = 0; k < G; ++k) *reinterpret_cast<f32x4 *>(s.pre + ip + (size_t)k * R) = acc[k];
            }
        }
        *reinterpret_cast<f32x4 *>(s.out + io) = o;
        if (s.out_a) {                                 // the logit GEMM's operand: out_res adds h_att BEFORE the dropout (AoAModel.py:181-185)
            f32x4 v = s.resid ? o + *reinterpret_cast<const f32x4 *>(s.resid + io) : o;
            if (s.mask_a) v *= *reinterpret_cast<const f32x4 *>(s.mask_a + io);
            *reinterpret_cast<f32x4 *>(s.out_a + io) = v;
            if (pl_a) pl_store4(pl_a, r, c, v);
        }
        if (s.out_b) {                                 // the NEXT step's context input: state[0][1], without the residual (:175-179)
            const f32x4 v = s.mask_b ? o * *reinterpret_cast<const f32x4 *>(s.mask_b + io) : o;
            *reinterpret_cast<f32x4 *>(s.out_b + io) = v;
            if (pl_b) pl_store4(pl_b, r, c, v);
        }
    }
}

// d_pre [M,R] of Linear -> ReLU from the gradient at its output: g = d_out + add_mask * sum_s add_slabs[s] (glu_bwd_kernel's order:
// slabs from 0.f, 8 per trip, the mask, then the sum), passed where the saved output is positive (relu_scale_bwd_kernel's test)
__global__ void relu_bwd_add_kernel(const float *__restrict__ d_out, const float *__restrict__ add_slabs, int add_splits,
                                    size_t add_stride, const float *__restrict__ add_mask, const float *__restrict__ out,
                                    float *__restrict__ d_pre, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float g = d_out[i];
        if (add_slabs) {
            float v = 0.f;
            for (int s0 = 0; s0 < add_splits; s0 += 8) {
                float tv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) tv[u] = s0 + u < add_splits ? add_slabs[(size_t)(s0 + u) * add_stride + i] : 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) v += tv[u];
            }
            if (add_mask) v *= add_mask[i];
            g = v + g;
        }
        d_pre[i] = out[i] > 0.f ? g : 0.f;
    }
}

}  // namespace

extern "C" {

int capmi_ctx_fwd_fused(const capmi_ctx_step *s, void *stream) {
    if (!s || !s->slabs || !s->out || s->splits < 1 || s->M <= 0 || s->R <= 0 || s->R % 4 || s->stride % 4) return CAPMI_EINVAL;
    if (s->kind != CAPMI_CTX_GLU && s->kind != CAPMI_CTX_RELU && s->kind != CAPMI_CTX_LSTM) return CAPMI_EINVAL;
    const int G = s->kind == CAPMI_CTX_RELU ? 1 : s->kind == CAPMI_CTX_GLU ? 2 : 4;
    if (s->splits > 1 && s->stride < (int64_t)s->M * G * s->R) return CAPMI_EINVAL;
    if (s->kind == CAPMI_CTX_GLU && !s->pre) return CAPMI_EINVAL;
    if (s->kind == CAPMI_CTX_LSTM && (!s->c_prev || !s->c)) return CAPMI_EINVAL;
    if ((s->planes_a || s->planes_b) && s->M > 64) return CAPMI_EINVAL;
    if ((s->planes_a && !s->out_a) || (s->planes_b && !s->out_b) || (s->resid && !s->out_a)) return CAPMI_EINVAL;
    if (!aligned16(s->slabs, s->bias, s->bias2, s->pre, s->c_prev, s->c, s->out, s->resid, s->mask_a, s->out_a, s->mask_b, s->out_b) ||
        ((reinterpret_cast<uintptr_t>(s->planes_a) | reinterpret_cast<uintptr_t>(s->planes_b)) & 15))
        return CAPMI_EINVAL;
    const dim3 grid(grid_for((size_t)s->M * (s->R / 4), 256, 4096));
    if (G == 1) hipLaunchKernelGGL(ctx_fwd_fused_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, *s);
    else if (G == 2) hipLaunchKernelGGL(ctx_fwd_fused_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, *s);
    else hipLaunchKernelGGL(ctx_fwd_fused_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, *s);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_relu_bwd_add(const float *d_out, const float *add_slabs, int add_splits, int64_t add_stride, const float *add_mask,
                       const float *out, float *d_pre, int M, int R, void *stream) {
    if (!d_out || !out || !d_pre || M <= 0 || R <= 0) return CAPMI_EINVAL;
    if (add_slabs && (add_splits < 1 || (add_splits > 1 && add_stride < (int64_t)M * R))) return CAPMI_EINVAL;
    hipLaunchKernelGGL(relu_bwd_add_kernel, dim3(grid_for((size_t)M * R, 256, 4096)), dim3(256), 0, (hipStream_t)stream, d_out, add_slabs,
                       add_splits, (size_t)add_stride, add_mask, out, d_pre, (size_t)M * R);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
