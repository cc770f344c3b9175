// Fused value clip + optimizer update on the flat fp32 buffer for the rules of misc.build_optimizer other than Adam
// (misc.py:114-130): RMSprop, Adagrad, SGD with momentum (plain and Nesterov), AdamW.  Adam itself stays in pointwise.hip
// (capmi_adam_step / capmi_adam_step_dyn), untouched.
//
// Element-wise and HBM bound: every stream (p, g, one or two state buffers) is read once and written once per step with 16-byte
// accesses, two independent quads per trip, grid-stride, no LDS.  The gradient and the state buffers are not read again before the
// next optimizer step, so they go non-temporal and the updated parameters are what stays in the Infinity Cache (as adam2_kernel
// does).  A range that does not start on a 16-byte boundary (a shard or bucket of the flat buffer) gets a scalar head of up to 3
// elements, any count a scalar tail of up to 3; buffers whose misalignments differ run scalar throughout.
//
// Everything derived from the learning rate and the step number is computed INSIDE the kernel, after the _dyn form has replaced
// them by the words of the device step record: the stepped and the captured form are the same arithmetic on the same floats.
//
// The exponential moving average of the parameters (capmi_ema_step / capmi_ema_step_dyn, --ema_decay) is a pass of its own in the
// same shape: p read once (plain: the optimizer has just written it and the next forward streams it), ema read and written once,
// non-temporal -- nothing reads the average before the next step.  12 bytes per element.
#include "host_common.h"

using namespace capmi;

namespace {

struct OptimArgs {
    float lr, a, b, eps, wd, clip, gscale, bc1, bc2_sqrt;
    int first;      // step == 1: torch.optim.SGD initialises the momentum buffer to the gradient
};

struct OptimDerived {
    float lr, a, b, eps, wd, clip, gscale, bc2_sqrt, step_size, decay;
    bool first;
};

__device__ __forceinline__ OptimDerived derive(OptimArgs h, const capmi_step_state *dyn) {
    if (dyn) { h.lr = dyn->lr; h.bc1 = dyn->bc1; h.bc2_sqrt = dyn->bc2_sqrt; h.first = dyn->adam_step == 1; }
    OptimDerived d;
    d.lr = h.lr; d.a = h.a; d.b = h.b; d.eps = h.eps; d.wd = h.wd; d.clip = h.clip; d.gscale = h.gscale; d.bc2_sqrt = h.bc2_sqrt;
    d.step_size = h.lr / h.bc1;            // AdamW
    d.decay = 1.f - h.lr * h.wd;           // AdamW: p *= 1 - lr * wd
    d.first = h.first != 0;
    return d;
}

// one element.  x: the raw gradient; s1 / s2: the rule's state (s2: AdamW only)
template <int RULE>
__device__ __forceinline__ void update(float &p, float x, float &s1, float &s2, const OptimDerived &d) {
    x *= d.gscale;
    if (d.clip > 0.f) x = fminf(fmaxf(x, -d.clip), d.clip);
    if (RULE == CAPMI_OPTIM_ADAMW) {
        // torch.optim.AdamW: decoupled decay, then Adam without an L2 term
        p *= d.decay;
        s1 = d.a * s1 + (1.f - d.a) * x;
        s2 = d.b * s2 + (1.f - d.b) * x * x;
        p -= d.step_size * s1 / (sqrtf(s2) / d.bc2_sqrt + d.eps);
        return;
    }
    if (d.wd != 0.f) x += d.wd * p;         // L2 folded into the gradient
    if (RULE == CAPMI_OPTIM_RMSPROP) {      // torch.optim.RMSprop, not centred, no momentum
        s1 = d.a * s1 + (1.f - d.a) * x * x;
        p -= d.lr * x / (sqrtf(s1) + d.eps);
    } else if (RULE == CAPMI_OPTIM_ADAGRAD) {   // torch.optim.Adagrad, lr_decay 0
        s1 += x * x;
        p -= d.lr * x / (sqrtf(s1) + d.eps);
    } else {                                // torch.optim.SGD, dampening 0
        s1 = d.first ? x : d.a * s1 + x;
        p -= d.lr * (RULE == CAPMI_OPTIM_SGDMOM ? x + d.a * s1 : s1);
    }
}

// elements [0, head) and [head + 4 * quads, count) scalar, the quads between them 16 bytes at a time
template <int RULE>
__global__ void optim_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ s1, float *__restrict__ s2,
                             size_t head, size_t quads, size_t count, OptimArgs args, const capmi_step_state *__restrict__ dyn) {
    constexpr bool TWO = RULE == CAPMI_OPTIM_ADAMW;
    const OptimDerived d = derive(args, dyn);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g + head);
    f32x4 *p4 = reinterpret_cast<f32x4 *>(p + head), *a4 = reinterpret_cast<f32x4 *>(s1 + head);
    f32x4 *b4 = TWO ? reinterpret_cast<f32x4 *>(s2 + head) : nullptr;
    for (size_t q0 = tid; q0 < quads; q0 += 2 * stride) {
        const size_t q1 = q0 + stride;
        const bool two = q1 < quads;
        const size_t q1c = two ? q1 : q0;
        f32x4 gg[2], pp[2], aa[2], bb[2];
        gg[0] = __builtin_nontemporal_load(g4 + q0); gg[1] = __builtin_nontemporal_load(g4 + q1c);
        aa[0] = __builtin_nontemporal_load(a4 + q0); aa[1] = __builtin_nontemporal_load(a4 + q1c);
        if (TWO) { bb[0] = __builtin_nontemporal_load(b4 + q0); bb[1] = __builtin_nontemporal_load(b4 + q1c); }
        else { bb[0] = f32x4{0.f, 0.f, 0.f, 0.f}; bb[1] = bb[0]; }
        pp[0] = p4[q0]; pp[1] = p4[q1c];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pp[u][k], ak = aa[u][k], bk = bb[u][k];
                update<RULE>(pk, gg[u][k], ak, bk, d);
                pp[u][k] = pk; aa[u][k] = ak; bb[u][k] = bk;
            }
        p4[q0] = pp[0];
        __builtin_nontemporal_store(aa[0], a4 + q0);
        if (TWO) __builtin_nontemporal_store(bb[0], b4 + q0);
        if (two) {
            p4[q1] = pp[1];
            __builtin_nontemporal_store(aa[1], a4 + q1);
            if (TWO) __builtin_nontemporal_store(bb[1], b4 + q1);
        }
    }
    const size_t body_end = head + quads * 4;
    const size_t scalars = head + (count - body_end);
    for (size_t t = tid; t < scalars; t += stride) {
        const size_t i = t < head ? t : body_end + (t - head);
        float pk = p[i], ak = s1[i], bk = TWO ? s2[i] : 0.f;
        update<RULE>(pk, g[i], ak, bk, d);
        p[i] = pk; s1[i] = ak;
        if (TWO) s2[i] = bk;
    }
}

template <int RULE>
void launch(float *p, const float *g, float *s1, float *s2, size_t head, size_t quads, size_t count, const OptimArgs &a,
            const capmi_step_state *dyn, hipStream_t st) {
    const size_t scalars = count - quads * 4;
    const size_t work = quads / 2 + 1 > scalars ? quads / 2 + 1 : scalars;
    hipLaunchKernelGGL(optim_kernel<RULE>, dim3(grid_for(work)), dim3(256), 0, st, p, g, s1, s2, head, quads, count, a, dyn);
}

int optim_launch(const capmi_optim_hp *hp, float *p, const float *g, float *s1, float *s2, int64_t count, float lr, float bc1,
                 float bc2_sqrt, int first, const capmi_step_state *dyn, void *stream) {
    const bool two = hp->rule == CAPMI_OPTIM_ADAMW;
    const uintptr_t up = reinterpret_cast<uintptr_t>(p), ug = reinterpret_cast<uintptr_t>(g), u1 = reinterpret_cast<uintptr_t>(s1),
                    u2 = two ? reinterpret_cast<uintptr_t>(s2) : up;
    if ((up | ug | u1 | u2) & 3) return CAPMI_EINVAL;
    const size_t n = (size_t)count;
    size_t head = n;                                        // misalignments differ: no common quad grid, scalar throughout
    if ((up & 15) == (ug & 15) && (up & 15) == (u1 & 15) && (up & 15) == (u2 & 15)) {
        head = ((16 - (up & 15)) & 15) / 4;
        if (head > n) head = n;
    }
    const size_t quads = (n - head) / 4;
    const OptimArgs a{lr, hp->alpha, hp->beta, hp->eps, hp->weight_decay, hp->clip, hp->grad_scale, bc1, bc2_sqrt, first};
    hipStream_t st = (hipStream_t)stream;
    switch (hp->rule) {
    case CAPMI_OPTIM_RMSPROP: launch<CAPMI_OPTIM_RMSPROP>(p, g, s1, s2, head, quads, n, a, dyn, st); break;
    case CAPMI_OPTIM_ADAGRAD: launch<CAPMI_OPTIM_ADAGRAD>(p, g, s1, s2, head, quads, n, a, dyn, st); break;
    case CAPMI_OPTIM_SGDM: launch<CAPMI_OPTIM_SGDM>(p, g, s1, s2, head, quads, n, a, dyn, st); break;
    case CAPMI_OPTIM_SGDMOM: launch<CAPMI_OPTIM_SGDMOM>(p, g, s1, s2, head, quads, n, a, dyn, st); break;
    case CAPMI_OPTIM_ADAMW: launch<CAPMI_OPTIM_ADAMW>(p, g, s1, s2, head, quads, n, a, dyn, st); break;
    default: return CAPMI_EINVAL;
    }
    CAPMI_CHECK_LAUNCH();
    return 0;
}

bool valid(const capmi_optim_hp *hp, const float *p, const float *g, const float *s1, const float *s2, int64_t count) {
    if (!hp || !p || !g || !s1 || count <= 0) return false;
    if (hp->rule < CAPMI_OPTIM_RMSPROP || hp->rule > CAPMI_OPTIM_ADAMW) return false;
    return hp->rule != CAPMI_OPTIM_ADAMW || s2 != nullptr;
}

// ---- exponential moving average of the parameters ----------------------------------------------------------------------------
struct EmaArgs {
    float decay;
    int warmup, step;
};

// the decay of this step.  warmup: min(decay, (1 + step) / (10 + step)), so that the first steps are not averaged against the initial
// weights for 1 / (1 - decay) steps
__device__ __forceinline__ float ema_decay(EmaArgs h, const capmi_step_state *dyn) {
    const int step = dyn ? dyn->adam_step : h.step;
    return h.warmup ? fminf(h.decay, (1.f + step) / (10.f + step)) : h.decay;
}

__device__ __forceinline__ float ema_update(float e, float p, float d, float om) { return fmaf(d, e, om * p); }

// elements [0, head) and [head + 4 * quads, count) scalar, the quads between them 16 bytes at a time (as optim_kernel)
__global__ void ema_kernel(float *__restrict__ ema, const float *__restrict__ p, size_t head, size_t quads, size_t count, EmaArgs args,
                           const capmi_step_state *__restrict__ dyn) {
    const float d = ema_decay(args, dyn);
    const float om = 1.f - d;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const f32x4 *p4 = reinterpret_cast<const f32x4 *>(p + head);
    f32x4 *e4 = reinterpret_cast<f32x4 *>(ema + head);
    for (size_t q0 = tid; q0 < quads; q0 += 2 * stride) {
        const size_t q1 = q0 + stride;
        const bool two = q1 < quads;
        const size_t q1c = two ? q1 : q0;
        f32x4 ee[2], pp[2];
        ee[0] = __builtin_nontemporal_load(e4 + q0); ee[1] = __builtin_nontemporal_load(e4 + q1c);
        pp[0] = p4[q0]; pp[1] = p4[q1c];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) ee[u][k] = ema_update(ee[u][k], pp[u][k], d, om);
        __builtin_nontemporal_store(ee[0], e4 + q0);
        if (two) __builtin_nontemporal_store(ee[1], e4 + q1);
    }
    const size_t body_end = head + quads * 4;
    const size_t scalars = head + (count - body_end);
    for (size_t t = tid; t < scalars; t += stride) {
        const size_t i = t < head ? t : body_end + (t - head);
        ema[i] = ema_update(ema[i], p[i], d, om);
    }
}

bool ema_valid(const float *ema, const float *p, int64_t count, float decay) {
    if (!ema || !p || ema == p || count <= 0) return false;
    if (!(decay >= 0.f && decay < 1.f)) return false;
    return ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(p)) & 3) == 0;
}

int ema_launch(float *ema, const float *p, int64_t count, float decay, int warmup, int step, const capmi_step_state *dyn, void *stream) {
    const uintptr_t ue = reinterpret_cast<uintptr_t>(ema), up = reinterpret_cast<uintptr_t>(p);
    const size_t n = (size_t)count;
    size_t head = n;                                        // misalignments differ: no common quad grid, scalar throughout
    if ((ue & 15) == (up & 15)) {
        head = ((16 - (ue & 15)) & 15) / 4;
        if (head > n) head = n;
    }
    const size_t quads = (n - head) / 4;
    const size_t scalars = n - quads * 4;
    const size_t work = quads / 2 + 1 > scalars ? quads / 2 + 1 : scalars;
    const EmaArgs a{decay, warmup != 0, step};
    hipLaunchKernelGGL(ema_kernel, dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, ema, p, head, quads, n, a, dyn);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int capmi_optim_step(const capmi_optim_hp *hp, float *p, const float *g, float *s1, float *s2, int64_t count, float lr, int step,
                     void *stream) {
    if (!valid(hp, p, g, s1, s2, count) || step < 1) return CAPMI_EINVAL;
    float bc1 = 1.f, bc2_sqrt = 1.f;
    if (hp->rule == CAPMI_OPTIM_ADAMW) {                    // double arithmetic, like capmi_adam_step and capmi_step_advance
        bc1 = (float)(1.0 - pow((double)hp->alpha, step));
        bc2_sqrt = (float)sqrt(1.0 - pow((double)hp->beta, step));
    }
    return optim_launch(hp, p, g, s1, s2, count, lr, bc1, bc2_sqrt, step == 1, nullptr, stream);
}

int capmi_optim_step_dyn(const capmi_optim_hp *hp, float *p, const float *g, float *s1, float *s2, int64_t count,
                         const capmi_step_state *state, void *stream) {
    if (!valid(hp, p, g, s1, s2, count) || !state) return CAPMI_EINVAL;
    return optim_launch(hp, p, g, s1, s2, count, 0.f, 1.f, 1.f, 0, state, stream);
}

int capmi_ema_step(float *ema, const float *p, int64_t count, float decay, int warmup, int step, void *stream) {
    if (!ema_valid(ema, p, count, decay) || step < 1) return CAPMI_EINVAL;
    return ema_launch(ema, p, count, decay, warmup, step, nullptr, stream);
}

int capmi_ema_step_dyn(float *ema, const float *p, int64_t count, const capmi_step_state *state, float decay, int warmup, void *stream) {
    if (!ema_valid(ema, p, count, decay) || !state) return CAPMI_EINVAL;
    return ema_launch(ema, p, count, decay, warmup, 0, state, stream);
}

}  // extern "C"
