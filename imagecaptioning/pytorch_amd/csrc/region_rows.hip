// Store rows of newly inserted images, built on the device (captioning/data/resident.py): what the reference's
// Dataset.__getitem__ does per image on the host (captioning/data/dataloader.py:266-282) -- norm_att_feat, the five box-geometry
// columns of use_box, norm_box_feat, the append and the re-ordering of the K rows by the last column, descending and stable.
//
// One launch per block of images, one workgroup per image, three phases:
//   1. geometry: one thread per region forms x1/w, y1/h, x2/w, y2/h, ((x2-x1)*(y2-y1))/(w*h) with correctly rounded, non-contracted
//      float32 operations in the reference's order (w, h and the integer product w*h converted to float first), optionally divides
//      the 5-vector by its L2 norm (squares summed left to right), and leaves the five columns and the key (the last one) in LDS.
//      The area is a sort key: an fma contraction or an approximate reciprocal could flip two rows, so none is used and the file
//      is compiled with -ffp-contract=off (build.py).
//   2. order: rank(i) = #{j : key_j > key_i or (key_j == key_i and j < i)}, counted by one thread per region over the keys in LDS --
//      the position Python's stable sorted(..., reverse=True) gives row i.
//      NaN keys: Python's sorted compares with `<`, which is false on both sides of a NaN, so its result depends on where the NaNs
//      stand and is no order a rank can restate.  Here the order is total: every non-NaN key (infinities included) in front, descending;
//      the NaN keys (a zero-norm box under norm_box, non-finite input) behind them in file order.  Every row is written exactly once
//      whatever the keys are.  Refusing a non-finite key would need the host to wait for the kernel; it is not refused.
//   3. rows: one wave per region row.  With norm_att the wave first sums the squares of the row (each lane its quads in order, then the
//      fixed wave butterfly of capmi_common.h: deterministic, no atomics) and every element is divided by the root.  Row i goes to
//      row rank(i) of the destination.  A destination row of D + 5 floats is generally not 16-byte aligned (2053 * 4 = 4 mod 16), so
//      every row has a scalar head of up to 3 elements up to its first 16-byte boundary, 16-byte stores from there, and a scalar tail
//      of up to 3 (optim.hip's split, per row); no store is misaligned.  The source is read 16 bytes at a time where the quad's source
//      address allows, dword by dword otherwise.  Raw rows are never read again: the last read of an element is non-temporal (with
//      norm_att the sum of squares reads it plain first, and the second read is served by the cache).
// use_box == 0 skips phases 1 and 2 (rank(i) = i): norm_att alone, off the host.
#include "host_common.h"

using namespace capmi;

namespace {

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / CAPMI_WAVE;

struct RowsArgs {
    const float *src, *boxes;
    const int32_t *table;       // [n_images][4]: first row, K, height, width
    float *dst;
    int64_t ldd;
    int D, norm_att, use_box, norm_box;
};

// true when j stands in front of i in the output
__device__ __forceinline__ bool in_front(float kj, int j, float ki, int i) {
    const bool nj = kj != kj, ni = ki != ki;
    if (nj || ni) return nj == ni ? j < i : ni;
    return kj > ki || (kj == ki && j < i);
}

__global__ __launch_bounds__(THREADS) void region_rows_kernel(RowsArgs a) {
    __shared__ float box[CAPMI_REGION_KMAX * 5];
    __shared__ int rank[CAPMI_REGION_KMAX];
    const int32_t *t = a.table + 4 * (size_t)blockIdx.x;
    const int64_t first = t[0];
    const int K = t[1];
    const int D = a.D;
    if (a.use_box) {
        const float w = (float)t[3], h = (float)t[2], wh = (float)((int64_t)t[3] * (int64_t)t[2]);
        for (int i = threadIdx.x; i < K; i += THREADS) {
            const float *b = a.boxes + (first + i) * 4;
            const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
            float c[5] = {__fdiv_rn(x1, w), __fdiv_rn(y1, h), __fdiv_rn(x2, w), __fdiv_rn(y2, h),
                          __fdiv_rn(__fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1)), wh)};
            if (a.norm_box) {
                float s = __fmul_rn(c[0], c[0]);
#pragma unroll
                for (int e = 1; e < 5; ++e) s = __fadd_rn(s, __fmul_rn(c[e], c[e]));
                const float n = __builtin_sqrtf(s);             // correctly rounded; __fsqrt_rn is the native (approximate) root
#pragma unroll
                for (int e = 0; e < 5; ++e) c[e] = __fdiv_rn(c[e], n);
            }
#pragma unroll
            for (int e = 0; e < 5; ++e) box[i * 5 + e] = c[e];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < K; i += THREADS) {
            const float ki = box[i * 5 + 4];
            int r = 0;
            for (int j = 0; j < K; ++j) r += in_front(box[j * 5 + 4], j, ki, i) ? 1 : 0;
            rank[i] = r;
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & (CAPMI_WAVE - 1), wid = threadIdx.x / CAPMI_WAVE;
    const int W = D + (a.use_box ? 5 : 0);
    for (int i = wid; i < K; i += WAVES) {                      // wave-uniform
        const float *s = a.src + (first + i) * D;
        float nrm = 1.f;
        if (a.norm_att) {
            float acc = 0.f;
            if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
                const f32x4 *s4 = reinterpret_cast<const f32x4 *>(s);
                for (int q = lane; q < D / 4; q += CAPMI_WAVE) {
                    const f32x4 v = s4[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __fadd_rn(acc, __fmul_rn(v[e], v[e]));
                }
                for (int c = (D & ~3) + lane; c < D; c += CAPMI_WAVE) acc = __fadd_rn(acc, __fmul_rn(s[c], s[c]));
            } else {
                for (int c = lane; c < D; c += CAPMI_WAVE) acc = __fadd_rn(acc, __fmul_rn(s[c], s[c]));
            }
            nrm = __fsqrt_rn(wave_sum(acc));
        }
        const int ro = a.use_box ? rank[i] : i;
        float *o = a.dst + (first + ro) * a.ldd;
        const float *bx = box + i * 5;
        // output column c: a (scaled) feature, or a geometry column
        auto val = [&](int c) -> float {
            if (c >= D) return bx[c - D];
            const float x = __builtin_nontemporal_load(s + c);
            return a.norm_att ? __fdiv_rn(x, nrm) : x;
        };
        int head = (int)(((16 - (reinterpret_cast<uintptr_t>(o) & 15)) & 15) >> 2);
        if (head > W) head = W;
        const int quads = (W - head) / 4;
        const bool src16 = (reinterpret_cast<uintptr_t>(s + head) & 15) == 0;
        f32x4 *o4 = reinterpret_cast<f32x4 *>(o + head);
        for (int q = lane; q < quads; q += CAPMI_WAVE) {
            const int c = head + 4 * q;
            f32x4 v;
            if (src16 && c + 4 <= D) {
                v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(s + c));
                if (a.norm_att) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = __fdiv_rn(v[e], nrm);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = val(c + e);
            }
            o4[q] = v;
        }
        const int body_end = head + 4 * quads;
        const int scalars = head + (W - body_end);              // <= 6
        if (lane < scalars) {
            const int c = lane < head ? lane : body_end + (lane - head);
            o[c] = val(c);
        }
    }
}

}  // namespace

extern "C" {

int capmi_region_rows_build(const float *src, const float *boxes, const int32_t *table_host, const int32_t *table, int n_images,
                            int D, float *dst, int64_t ldd, int norm_att, int use_box, int norm_box, void *stream) {
    if (!src || !table_host || !table || !dst || n_images <= 0 || D <= 0) return CAPMI_EINVAL;
    if (use_box && !boxes) return CAPMI_EINVAL;
    if (ldd < (int64_t)D + (use_box ? 5 : 0)) return CAPMI_EINVAL;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(dst) |
         reinterpret_cast<uintptr_t>(table)) & 3)
        return CAPMI_EINVAL;
    for (int i = 0; i < n_images; ++i) {
        const int32_t *t = table_host + 4 * (size_t)i;
        if (t[0] < 0 || t[1] <= 0) return CAPMI_EINVAL;
        if (use_box && (t[1] > CAPMI_REGION_KMAX || t[2] <= 0 || t[3] <= 0)) return CAPMI_EINVAL;
    }
    const RowsArgs a{src, boxes, table, dst, ldd, D, norm_att != 0, use_box != 0, (use_box && norm_box) ? 1 : 0};
    hipLaunchKernelGGL(region_rows_kernel, dim3(n_images), dim3(THREADS), 0, (hipStream_t)stream, a);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
