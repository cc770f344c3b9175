// The compact resident feature store (captioning/data/resident.py): region rows kept as bf16 or fp16, and the launch that turns the
// store into a batch.
//
// rows_narrow_kernel: fp32 -> bf16 / fp16, round to nearest even, element-wise.  The destination is any 2-byte-aligned place of the
//   store, so the launch is split like optim.hip's: a scalar head of up to 7 elements up to the first 16-byte boundary of dst,
//   16-byte stores of 8 elements from there (grid-stride), and a scalar tail of up to 7.  The source block is read 2 x 16 bytes per
//   trip where src + head is 16-byte aligned, dword by dword otherwise; it is a staging block that is never read again, so its
//   loads are non-temporal.
//     bf16: NaN keeps its sign and its upper payload bits and gets the quiet bit; everything else is u + 0x7fff + (bit 16 of u)
//           cut to the upper half -- the carry rounds the largest finite values to inf, which is round to nearest even.
//     fp16: the hardware conversion (v_cvt_f16_f32 in the default mode: nearest even, overflow to inf, fp16 subnormals produced;
//           fp16 denormals are never flushed on gfx950 code objects).
//
// gather_kernel: one workgroup per output row (b, k).  k < K copies store row first + k widened to fp32, k >= K writes zeros; thread
//   0 writes the mask word.  Widening is exact (bf16: the bits shifted up; fp16: v_cvt_f32_f16), so the output is a function of the
//   stored bits alone.  The split follows the OUTPUT row, the wider side: a scalar head of up to 3 floats, 16-byte stores of 4, a
//   scalar tail of up to 3 (an output row of F = 2053 floats starts 4 bytes further off a 16-byte boundary than its predecessor).
//   The 4 source elements of a quad are one load where the quad's source address allows -- 8 bytes for a 2-byte store, 16 for an
//   fp32 one --, two 4-byte loads where a 2-byte quad is 4-byte aligned, and single elements otherwise (a row of 2053 bf16 is 4106
//   bytes, so every second row of such a store starts 2 bytes off a dword).  The alignment class is uniform over the workgroup.
//
// rows_l2norm_kernel: norm_att_feat for rows that are about to enter the store, in place, one wave per row: x / sqrt(sum x * x) with the
//   sum taken in the order of numpy's float32 add.reduce, so that a store built on the device holds the bits the loader's host path
//   (feature_loader.finish_image: att / np.linalg.norm(att, 2, 1, keepdims=True)) produces.  That order: a run of n <= 128 elements is
//   summed by 8 accumulators striding the run (r_j = a_j + a_8+j + ...), combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)),
//   then the n % 8 tail elements are added one by one; a longer run is split at n / 2 rounded down to a multiple of 8 and the halves'
//   sums are added.  The split depends on D alone, so the host writes the leaves (offset, length) and the post-order add program into
//   the kernel arguments.  On the device 8 lanes own a leaf (lane j accumulator j; the xor-1, -2, -4 butterfly is the combine above),
//   8 leaves run at a time, and lane 0 replays the add program over the leaf sums in LDS.  Products, sums, root and quotient are
//   single correctly rounded float32 operations: the file is compiled with -ffp-contract=off (build.py), as region_rows.hip is.
#include "host_common.h"

using namespace capmi;

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int THREADS = 256;

template <int DT>
__device__ __forceinline__ uint16_t narrow(float x) {
    if (DT == CAPMI_ROWS_BF16) {
        const uint32_t u = __builtin_bit_cast(uint32_t, x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    return __builtin_bit_cast(uint16_t, (_Float16)x);
}

template <int DT>
__device__ __forceinline__ float widen(uint16_t h) {
    if (DT == CAPMI_ROWS_BF16) return __builtin_bit_cast(float, (uint32_t)h << 16);
    return (float)__builtin_bit_cast(_Float16, h);
}

template <int DT>
__global__ __launch_bounds__(THREADS) void rows_narrow_kernel(const float *__restrict__ src, uint16_t *__restrict__ dst, int64_t count) {
    int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 1);
    if (head > count) head = count;
    const int64_t trips = (count - head) / 8;
    const float *s = src + head;
    u32x4 *d4 = reinterpret_cast<u32x4 *>(dst + head);          // 16-byte aligned (or trips == 0)
    const bool src16 = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < trips; t += stride) {
        float v[8];
        if (src16) {
            const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(s + 8 * t));
            const f32x4 b = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(s + 8 * t) + 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = __builtin_nontemporal_load(s + 8 * t + e);
        }
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (uint32_t)narrow<DT>(v[2 * e]) | ((uint32_t)narrow<DT>(v[2 * e + 1]) << 16);
        d4[t] = o;
    }
    if (blockIdx.x == 0) {
        const int64_t body_end = head + 8 * trips;
        const int scalars = (int)(head + (count - body_end));   // <= 14
        if ((int)threadIdx.x < scalars) {
            const int64_t c = (int64_t)threadIdx.x < head ? (int64_t)threadIdx.x : body_end + ((int64_t)threadIdx.x - head);
            dst[c] = narrow<DT>(src[c]);
        }
    }
}

// 4 consecutive store elements as floats; cls: what the address of the quad allows (uniform over the workgroup)
//   16-bit stores: 0 = one 8-byte load, 1 = two 4-byte loads, 2 = four 2-byte loads;  fp32: 0 = one 16-byte load, else four dwords
template <int DT>
__device__ __forceinline__ f32x4 load_quad(const void *p, int cls) {
    f32x4 v;
    if (DT == CAPMI_ROWS_F32) {
        const float *s = reinterpret_cast<const float *>(p);
        if (cls == 0) return *reinterpret_cast<const f32x4 *>(s);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s[e];
        return v;
    }
    const uint16_t *s = reinterpret_cast<const uint16_t *>(p);
    uint32_t lo, hi;
    if (cls == 0) {
        const u32x2 w = *reinterpret_cast<const u32x2 *>(s);
        lo = w[0]; hi = w[1];
    } else if (cls == 1) {
        lo = reinterpret_cast<const uint32_t *>(s)[0];
        hi = reinterpret_cast<const uint32_t *>(s)[1];
    } else {
        lo = (uint32_t)s[0] | ((uint32_t)s[1] << 16);
        hi = (uint32_t)s[2] | ((uint32_t)s[3] << 16);
    }
    v[0] = widen<DT>((uint16_t)(lo & 0xffffu)); v[1] = widen<DT>((uint16_t)(lo >> 16));
    v[2] = widen<DT>((uint16_t)(hi & 0xffffu)); v[3] = widen<DT>((uint16_t)(hi >> 16));
    return v;
}

template <int DT>
__device__ __forceinline__ float load_one(const void *p, int c) {
    if (DT == CAPMI_ROWS_F32) return reinterpret_cast<const float *>(p)[c];
    return widen<DT>(reinterpret_cast<const uint16_t *>(p)[c]);
}

template <int DT>
__global__ __launch_bounds__(THREADS) void gather_kernel(const void *__restrict__ rows, int F, const int32_t *__restrict__ table, int kmax,
                                                         float *__restrict__ att, float *__restrict__ mask) {
    constexpr int ES = DT == CAPMI_ROWS_F32 ? 4 : 2;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / kmax, k = blockIdx.x - b * kmax;
    const int64_t first = table[2 * b];
    const int K = table[2 * b + 1];
    const bool live = k < K;
    float *o = att + (int64_t)blockIdx.x * F;
    if (tid == 0) mask[blockIdx.x] = live ? 1.f : 0.f;
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(o) & 15)) & 15) >> 2);
    if (head > F) head = F;
    const int quads = (F - head) / 4;
    const int body_end = head + 4 * quads;
    const int scalars = head + (F - body_end);                  // <= 6
    f32x4 *o4 = reinterpret_cast<f32x4 *>(o + head);
    if (!live) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int q = tid; q < quads; q += THREADS) o4[q] = z;
        if (tid < scalars) o[tid < head ? tid : body_end + (tid - head)] = 0.f;
        return;
    }
    const char *s = reinterpret_cast<const char *>(rows) + (first + k) * (int64_t)F * ES;
    const uintptr_t a = reinterpret_cast<uintptr_t>(s + (int64_t)head * ES);
    const int cls = DT == CAPMI_ROWS_F32 ? ((a & 15) ? 1 : 0) : ((a & 7) == 0 ? 0 : (a & 3) == 0 ? 1 : 2);
    for (int q = tid; q < quads; q += THREADS) o4[q] = load_quad<DT>(s + (int64_t)(head + 4 * q) * ES, cls);
    if (tid < scalars) {
        const int c = tid < head ? tid : body_end + (tid - head);
        o[c] = load_one<DT>(s, c);
    }
}

constexpr int NORM_LEAVES = 128;           // D <= CAPMI_ROWS_L2NORM_DMAX: every leaf but the only one of a short row holds 64..128 elements

struct NormPlan {
    uint16_t off[NORM_LEAVES];
    uint8_t len[NORM_LEAVES];              // length - 1
    uint8_t prog[2 * NORM_LEAVES];         // post order: 0 = push the next leaf sum, 1 = add the two on top
    int n_leaves, n_prog;
};

void plan_run(NormPlan &p, int off, int n) {
    if (n <= 128) {
        p.off[p.n_leaves] = (uint16_t)off;
        p.len[p.n_leaves++] = (uint8_t)(n - 1);
        p.prog[p.n_prog++] = 0;
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    plan_run(p, off, n2);
    plan_run(p, off + n2, n - n2);
    p.prog[p.n_prog++] = 1;
}

__global__ __launch_bounds__(CAPMI_WAVE) void rows_l2norm_kernel(float *__restrict__ rows, int D, NormPlan p) {
    __shared__ float leaf_sum[NORM_LEAVES];
    __shared__ float stack[16];
    float *x = rows + (int64_t)blockIdx.x * D;
    const int lane = threadIdx.x, j = lane & 7;
    for (int base = 0; base < p.n_leaves; base += 8) {
        const int i = base + (lane >> 3);
        const bool mine = i < p.n_leaves;
        const int off = mine ? p.off[i] : 0, n = mine ? p.len[i] + 1 : 0;
        const int body = n - n % 8;
        float r = 0.f;
        if (body) {
            const float a = x[off + j];
            r = __fmul_rn(a, a);
            for (int s = 8; s < body; s += 8) {
                const float b = x[off + s + j];
                r = __fadd_rn(r, __fmul_rn(b, b));
            }
        }
        r = __fadd_rn(r, __shfl_xor(r, 1));
        r = __fadd_rn(r, __shfl_xor(r, 2));
        r = __fadd_rn(r, __shfl_xor(r, 4));
        if (mine && j == 0) {
            for (int c = body; c < n; ++c) {                     // n < 8: numpy starts from 0 and adds one by one
                const float b = x[off + c];
                r = __fadd_rn(r, __fmul_rn(b, b));
            }
            leaf_sum[i] = r;
        }
    }
    __syncthreads();
    if (lane == 0) {
        int sp = 0, li = 0;
        for (int t = 0; t < p.n_prog; ++t) {
            if (p.prog[t] == 0) {
                stack[sp++] = leaf_sum[li++];
            } else {
                sp -= 1;
                stack[sp - 1] = __fadd_rn(stack[sp - 1], stack[sp]);
            }
        }
        stack[0] = __builtin_sqrtf(stack[0]);          // correctly rounded (__fsqrt_rn is the native, approximate root)
    }
    __syncthreads();
    const float nrm = stack[0];
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && D % 4 == 0) {
        f32x4 *x4 = reinterpret_cast<f32x4 *>(x);
        for (int q = lane; q < D / 4; q += CAPMI_WAVE) {
            f32x4 v = x4[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __fdiv_rn(v[e], nrm);
            x4[q] = v;
        }
    } else {
        for (int c = lane; c < D; c += CAPMI_WAVE) x[c] = __fdiv_rn(x[c], nrm);
    }
}

}  // namespace

extern "C" {

int capmi_rows_l2norm(float *rows, int64_t n_rows, int D, void *stream) {
    if (!rows || n_rows <= 0 || n_rows > 0x7fffffffLL || D <= 0 || D > CAPMI_ROWS_L2NORM_DMAX) return CAPMI_EINVAL;
    if (reinterpret_cast<uintptr_t>(rows) & 3) return CAPMI_EINVAL;
    NormPlan p{};
    plan_run(p, 0, D);
    hipLaunchKernelGGL(rows_l2norm_kernel, dim3((unsigned)n_rows), dim3(CAPMI_WAVE), 0, (hipStream_t)stream, rows, D, p);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_rows_narrow(const float *src, void *dst, int64_t count, int dtype, void *stream) {
    if (!src || !dst || count <= 0) return CAPMI_EINVAL;
    if (dtype != CAPMI_ROWS_BF16 && dtype != CAPMI_ROWS_FP16) return CAPMI_EINVAL;
    if ((reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(dst) & 1)) return CAPMI_EINVAL;
    const int grid = grid_for((size_t)(count / 8 + 1), THREADS);
    if (dtype == CAPMI_ROWS_BF16)
        hipLaunchKernelGGL(rows_narrow_kernel<CAPMI_ROWS_BF16>, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, src, (uint16_t *)dst, count);
    else
        hipLaunchKernelGGL(rows_narrow_kernel<CAPMI_ROWS_FP16>, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, src, (uint16_t *)dst, count);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

int capmi_resident_gather(const void *rows, int dtype, int F, const int32_t *table_host, const int32_t *table, int B, int kmax,
                          float *att, float *mask, void *stream) {
    if (!rows || !table_host || !table || !att || !mask || B <= 0 || kmax <= 0 || F <= 0) return CAPMI_EINVAL;
    if (dtype != CAPMI_ROWS_F32 && dtype != CAPMI_ROWS_BF16 && dtype != CAPMI_ROWS_FP16) return CAPMI_EINVAL;
    if ((int64_t)B * kmax > 0x7fffffffLL) return CAPMI_EINVAL;
    if ((reinterpret_cast<uintptr_t>(rows) & (dtype == CAPMI_ROWS_F32 ? 3 : 1)) ||
        ((reinterpret_cast<uintptr_t>(att) | reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(table)) & 3))
        return CAPMI_EINVAL;
    for (int b = 0; b < B; ++b) {
        const int32_t first = table_host[2 * b], K = table_host[2 * b + 1];
        if (K < 0 || K > kmax || (K > 0 && first < 0)) return CAPMI_EINVAL;
    }
    const dim3 grid((unsigned)(B * kmax)), block(THREADS);
    if (dtype == CAPMI_ROWS_F32)
        hipLaunchKernelGGL(gather_kernel<CAPMI_ROWS_F32>, grid, block, 0, (hipStream_t)stream, rows, F, table, kmax, att, mask);
    else if (dtype == CAPMI_ROWS_BF16)
        hipLaunchKernelGGL(gather_kernel<CAPMI_ROWS_BF16>, grid, block, 0, (hipStream_t)stream, rows, F, table, kmax, att, mask);
    else
        hipLaunchKernelGGL(gather_kernel<CAPMI_ROWS_FP16>, grid, block, 0, (hipStream_t)stream, rows, F, table, kmax, att, mask);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
