// Corpus CIDEr, BLEU-1..4 and ROUGE-L on the GPU (gfx950): the Java-free metrics of coco-caption over token ids, for the
// validation pass that picks model-best.pth during SCST (eval_utils.language_eval -> lang_stats; formulas in include/capmi.h).
//
// Three kinds of launch.  Building (once per split): a workgroup per image inserts the image's distinct reference n-grams into an
// open-addressing table in HBM (atomicCAS on the key, atomicAdd on the count), then a workgroup per reference stores the four
// tf-idf norms, so that scoring never looks a reference n-gram up.  Adding (once per decoded batch): a workgroup per hypothesis
// row cooks the row in LDS -- one lane per (order, start position), as ciderd.hip does -- and walks the image's references once:
// the occurrences of each hypothesis n-gram in the reference feed the CIDEr dot product and BLEU's clip count together; then one
// wave per reference runs the LCS rows of ROUGE-L in registers (a row of the table is a prefix maximum across the lanes).
// Reducing: one workgroup sums the per-image integers as integers and the scores in a fixed order.
//
// All of it is latency bound (a few hundred hash probes and LDS compares per caption): the point is that the decoded rows never
// leave HBM and the host reads eight doubles per evaluation.
#include "capmi_common.h"
#include "ngram_common.h"
#include "../../../include/capmi.h"

namespace {

using capmi::df_lookup;
using capmi::mix64;
using capmi::ngram_tf;
using capmi::pack_ngram;

constexpr int LMAX = CAPMI_LANGEVAL_LMAX;   // max tokens per row: one wave holds a row
constexpr int NG = 4;                       // n-gram orders 1..4
constexpr int CT = NG * LMAX;               // one lane per (order, start position)
constexpr double BETA = 1.2;
static_assert(LMAX == CAPMI_WAVE, "a caption row is staged and measured by one wave");

// one token of a row (0 beyond its width); an id the 16-bit key fields cannot hold is reported and ends the caption
__device__ __forceinline__ int load_token(const int64_t *row, int w, int lane, int32_t *err) {
    const int64_t t = lane < w ? row[lane] : 0;
    if (t < 0 || t >= 65535) {
        atomicOr(err, CAPMI_LANGEVAL_E_TOKEN);
        return 0;
    }
    return (int)t;
}

// caption length of the row whose lane-th token is t: tokens before the first 0.  Whole wave.
__device__ __forceinline__ int caption_len(int t, int w, int lane) {
    const unsigned long long ends = __ballot(lane >= w || t == 0);
    return ends ? __builtin_ctzll(ends) : LMAX;
}

// row -> tok[LMAX], *len (LDS); every thread of the workgroup calls it, wave 0 works; ends with a barrier
__device__ __forceinline__ void stage_row(const int64_t *row, int w, int *tok, int *len, int32_t *err) {
    if (threadIdx.x < LMAX) {
        const int t = load_token(row, w, threadIdx.x, err);
        tok[threadIdx.x] = t;
        const int n = caption_len(t, w, threadIdx.x);
        if (threadIdx.x == 0) *len = n;
    }
    __syncthreads();
}

__device__ __forceinline__ void df_insert(uint64_t *keys, int32_t *counts, uint32_t cap, uint64_t key, int32_t *err) {
    uint32_t slot = (uint32_t)mix64(key) & (cap - 1);
    for (uint32_t probe = 0; probe < cap; ++probe) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(keys + slot), 0ULL, (unsigned long long)key);
        if (prev == 0ULL || prev == key) {
            atomicAdd(counts + slot, 1);
            return;
        }
        slot = (slot + 1) & (cap - 1);
    }
    atomicOr(err, CAPMI_LANGEVAL_E_TABLE_FULL);
}

// One workgroup per image.  An n-gram instance is inserted when no earlier (reference, position) of the image holds the same
// n-gram: the set of insertions is the same on every run, only their order -- hence the slots -- is not, and a lookup does not
// see the slots.
__global__ __launch_bounds__(CT) void langeval_df_kernel(capmi_langeval e) {
    __shared__ int tok_c[LMAX], tok_o[LMAX], len_s[2];
    __shared__ uint64_t key_c[CT], key_o[CT];
    const int tid = threadIdx.x, k = tid / LMAX, i = tid % LMAX;
    const int r0 = e.ref_off[blockIdx.x], r1 = e.ref_off[blockIdx.x + 1];
    for (int r = r0; r < r1; ++r) {
        stage_row(e.refs + (size_t)r * e.ref_w, e.ref_w, tok_c, &len_s[0], e.err);
        const int len = len_s[0];
        const bool valid = i + k + 1 <= len;
        const uint64_t key = valid ? pack_ngram(tok_c, i, k) : 0;
        key_c[tid] = key;
        __syncthreads();
        bool first = valid;
        if (valid) ngram_tf(&key_c[k * LMAX], len - k, key, i, first);
        for (int o = r0; o < r; ++o) {                       // the image's earlier references
            stage_row(e.refs + (size_t)o * e.ref_w, e.ref_w, tok_o, &len_s[1], e.err);
            const int lo = len_s[1];
            key_o[tid] = i + k + 1 <= lo ? pack_ngram(tok_o, i, k) : 0;
            __syncthreads();
            if (first)
                for (int j = 0; j < lo - k; ++j)
                    if (key_o[k * LMAX + j] == key) { first = false; break; }
            __syncthreads();
        }
        if (first) df_insert(e.table_keys, e.table_counts, e.table_cap, key, e.err);
        __syncthreads();
    }
}

__device__ __forceinline__ double idf_of(const capmi_langeval &e, uint64_t key, double log_n) {
    const int df = df_lookup(e.table_keys, e.table_counts, e.table_cap, key);
    return log_n - log(fmax(1.0, (double)df));
}

// per-order norm of vec[CT] (0 on the lanes that hold no distinct n-gram): threads 0..NG-1, fixed order
__device__ __forceinline__ double order_norm(const double *vec, int k) {
    double s = 0.0;
    for (int j = 0; j < LMAX; ++j) s += vec[k * LMAX + j] * vec[k * LMAX + j];
    return sqrt(s);
}

// One workgroup per reference: ref_norm [total_refs, 4].
__global__ __launch_bounds__(CT) void langeval_ref_norm_kernel(capmi_langeval e, double log_n) {
    __shared__ int tok[LMAX], len_s;
    __shared__ uint64_t keys[CT];
    __shared__ double vec[CT];
    const int tid = threadIdx.x, k = tid / LMAX, i = tid % LMAX, r = blockIdx.x;
    stage_row(e.refs + (size_t)r * e.ref_w, e.ref_w, tok, &len_s, e.err);
    const int len = len_s;
    const bool valid = i + k + 1 <= len;
    const uint64_t key = valid ? pack_ngram(tok, i, k) : 0;
    keys[tid] = key;
    __syncthreads();
    bool first = valid;
    int tf = 0;
    if (valid) tf = ngram_tf(&keys[k * LMAX], len - k, key, i, first);
    vec[tid] = first ? (double)tf * idf_of(e, key, log_n) : 0.0;
    __syncthreads();
    if (tid < NG) e.ref_norm[(size_t)r * NG + tid] = order_norm(vec, tid);
}

// One workgroup per hypothesis row.
__global__ __launch_bounds__(CT) void langeval_add_kernel(capmi_langeval e, const int64_t *__restrict__ hyp, int H, int L,
                                                         const int64_t *__restrict__ img_idx, double log_n) {
    __shared__ int tok_h[LMAX], tok_r[LMAX], len_s[2];
    __shared__ uint64_t key_h[CT], key_r[CT];
    __shared__ double contrib[CT], norm_h[NG], score[NG], wave_p[NG], wave_r[NG];
    __shared__ int icontrib[CT];
    const int h = blockIdx.x, tid = threadIdx.x, k = tid / LMAX, i = tid % LMAX;
    const int64_t img64 = img_idx[h];
    int later = 0;                                           // a later row of this call describes the same image: it counts
    for (int j = h + 1 + tid; j < H; j += CT) later |= img_idx[j] == img64;
    if (__syncthreads_or(later)) return;
    if (img64 < 0 || img64 >= e.n_img) {
        if (tid == 0) atomicOr(e.err, CAPMI_LANGEVAL_E_IMAGE);
        return;
    }
    const int img = (int)img64;
    const int r0 = e.ref_off[img], r1 = e.ref_off[img + 1];

    // ---- the hypothesis: distinct n-grams, their counts and tf-idf weights
    stage_row(hyp + (size_t)h * L, L, tok_h, &len_s[0], e.err);
    const int len_h = len_s[0];
    const bool valid = i + k + 1 <= len_h;
    const uint64_t key = valid ? pack_ngram(tok_h, i, k) : 0;
    key_h[tid] = key;
    __syncthreads();
    bool first = valid;
    int tf_h = 0;
    if (valid) tf_h = ngram_tf(&key_h[k * LMAX], len_h - k, key, i, first);
    const double idf = first ? idf_of(e, key, log_n) : 0.0;
    const double vh = (double)tf_h * idf;
    contrib[tid] = first ? vh : 0.0;
    __syncthreads();
    if (tid < NG) {
        norm_h[tid] = order_norm(contrib, tid);
        score[tid] = 0.0;
    }

    // ---- one walk over the references: CIDEr dot products, BLEU clip counts, the closest length
    int max_tf = 0, best_d = 1 << 30, best_l = 0;
    for (int r = r0; r < r1; ++r) {
        __syncthreads();                                     // contrib / tok_r / key_r of the previous reference are consumed
        stage_row(e.refs + (size_t)r * e.ref_w, e.ref_w, tok_r, &len_s[1], e.err);
        const int len_r = len_s[1];
        key_r[tid] = i + k + 1 <= len_r ? pack_ngram(tok_r, i, k) : 0;
        __syncthreads();
        int tf_r = 0;
        if (first)
            for (int j = 0; j < len_r - k; ++j) tf_r += key_r[k * LMAX + j] == key;
        max_tf = max(max_tf, tf_r);
        contrib[tid] = first ? vh * ((double)tf_r * idf) : 0.0;     // the reference's weight of the same n-gram: same idf
        __syncthreads();
        if (tid < NG) {
            double s = 0.0;
            for (int j = 0; j < LMAX; ++j) s += contrib[tid * LMAX + j];
            const double nh = norm_h[tid], nr = e.ref_norm[(size_t)r * NG + tid];
            if (nh != 0.0 && nr != 0.0) s /= nh * nr;
            score[tid] += s;
        }
        const int d = abs(len_r - len_h);
        if (d < best_d || (d == best_d && len_r < best_l)) { best_d = d; best_l = len_r; }
    }
    __syncthreads();
    icontrib[tid] = first ? min(tf_h, max_tf) : 0;
    __syncthreads();
    if (tid < NG) {
        int correct = 0;
        for (int j = 0; j < LMAX; ++j) correct += icontrib[tid * LMAX + j];
        e.bleu_stats[((size_t)img * NG + tid) * 2 + 0] = max(0, len_h - tid);
        e.bleu_stats[((size_t)img * NG + tid) * 2 + 1] = correct;
    }
    if (tid == 0) {
        double m = 0.0;
        for (int q = 0; q < NG; ++q) m += score[q];
        e.cider[img] = r1 > r0 ? m / NG / (double)(r1 - r0) * 10.0 : 0.0;
        e.lens[(size_t)img * 2 + 0] = len_h;
        e.lens[(size_t)img * 2 + 1] = best_l;
    }

    // ---- ROUGE-L: wave w takes references w, w + 4, ...; lane j holds column j + 1 of the LCS table's current row.
    // With x[j] = row[i-1][j-1] + 1 where the tokens match and row[i-1][j] elsewhere, row[i] is the prefix maximum of x.
    const int wave = tid / CAPMI_WAVE, lane = tid % CAPMI_WAVE;
    const int th = lane < len_h ? tok_h[lane] : -1;
    double p_max = 0.0, r_max = 0.0;
    for (int r = r0 + wave; r < r1; r += NG) {
        const int tr = load_token(e.refs + (size_t)r * e.ref_w, e.ref_w, lane, e.err);
        const int len_r = caption_len(tr, e.ref_w, lane);
        int row = 0;
        for (int a = 0; a < len_r; ++a) {
            const int ta = __shfl(tr, a);
            int diag = __shfl_up(row, 1);
            if (lane == 0) diag = 0;
            int x = th == ta ? diag + 1 : row;
#pragma unroll
            for (int o = 1; o < CAPMI_WAVE; o <<= 1) {
                const int y = __shfl_up(x, o);
                if (lane >= o) x = max(x, y);
            }
            row = x;
        }
        const int lcs = __shfl(row, CAPMI_WAVE - 1);         // columns past the hypothesis carry the last value on
        if (lane == 0) e.lcs[r] = lcs;
        if (len_h > 0) p_max = fmax(p_max, (double)lcs / (double)len_h);
        if (len_r > 0) r_max = fmax(r_max, (double)lcs / (double)len_r);
    }
    if (lane == 0) { wave_p[wave] = p_max; wave_r[wave] = r_max; }
    __syncthreads();
    if (tid == 0) {
        double p = 0.0, q = 0.0;
        for (int w = 0; w < NG; ++w) { p = fmax(p, wave_p[w]); q = fmax(q, wave_r[w]); }
        e.rouge[img] = (p != 0.0 && q != 0.0) ? (1.0 + BETA * BETA) * p * q / (q + BETA * BETA * p) : 0.0;
        e.seen[img] = 1;
    }
}

constexpr int NI = 10;    // integer totals: guess 1..4, correct 1..4, testlen, reflen
constexpr int RT = 256;

// One workgroup.  Every thread sums its images (stride RT), then one thread per quantity adds the RT partial sums in index order.
__global__ __launch_bounds__(RT) void langeval_reduce_kernel(capmi_langeval e, double *__restrict__ out, int64_t *__restrict__ totals) {
    __shared__ int64_t si[NI + 1][RT];
    __shared__ double sd[2][RT];
    __shared__ int64_t ti[NI + 1];
    __shared__ double td[2];
    const int tid = threadIdx.x;
    int64_t acc[NI + 1] = {};
    double c = 0.0, g = 0.0;
    for (int img = tid; img < e.n_img; img += RT) {
        if (!e.seen[img]) continue;
        for (int q = 0; q < NG; ++q) {
            acc[q] += e.bleu_stats[((size_t)img * NG + q) * 2 + 0];
            acc[NG + q] += e.bleu_stats[((size_t)img * NG + q) * 2 + 1];
        }
        acc[8] += e.lens[(size_t)img * 2 + 0];
        acc[9] += e.lens[(size_t)img * 2 + 1];
        acc[NI] += 1;
        c += e.cider[img];
        g += e.rouge[img];
    }
    for (int q = 0; q <= NI; ++q) si[q][tid] = acc[q];
    sd[0][tid] = c;
    sd[1][tid] = g;
    __syncthreads();
    if (tid <= NI) {
        int64_t s = 0;
        for (int j = 0; j < RT; ++j) s += si[tid][j];
        ti[tid] = s;
    } else if (tid < NI + 3) {
        double s = 0.0;
        for (int j = 0; j < RT; ++j) s += sd[tid - NI - 1][j];
        td[tid - NI - 1] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const double tiny = 1e-15, small = 1e-9;             // bleu_scorer.py
        const double ratio = ((double)ti[8] + tiny) / ((double)ti[9] + small);
        const double bp = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
        double bleu = 1.0;
        for (int q = 0; q < NG; ++q) {
            bleu *= ((double)ti[NG + q] + tiny) / ((double)ti[q] + small);
            out[q] = pow(bleu, 1.0 / (q + 1)) * bp;
        }
        const double n = (double)ti[NI];
        out[4] = n > 0 ? td[1] / n : 0.0;
        out[5] = n > 0 ? td[0] / n : 0.0;
        out[6] = n;
        out[7] = (double)*e.err;
        for (int q = 0; q < NI; ++q) totals[q] = ti[q];
    }
}

bool langeval_valid(const capmi_langeval *e) {
    if (!e || !e->refs || !e->ref_off || !e->table_keys || !e->table_counts || !e->ref_norm || !e->cider || !e->rouge ||
        !e->bleu_stats || !e->lens || !e->lcs || !e->seen || !e->err)
        return false;
    if (e->n_img < 1 || e->total_refs < 0 || e->ref_w < 1 || e->ref_w > LMAX) return false;
    return e->table_cap != 0 && !(e->table_cap & (e->table_cap - 1));
}

}  // namespace

extern "C" int capmi_langeval_build(const capmi_langeval *e, void *stream) {
    if (!langeval_valid(e)) return CAPMI_EINVAL;
    hipLaunchKernelGGL(langeval_df_kernel, dim3(e->n_img), dim3(CT), 0, (hipStream_t)stream, *e);
    CAPMI_CHECK_LAUNCH();
    if (e->total_refs > 0) {
        hipLaunchKernelGGL(langeval_ref_norm_kernel, dim3(e->total_refs), dim3(CT), 0, (hipStream_t)stream, *e, log((double)e->n_img));
        CAPMI_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int capmi_langeval_add(const capmi_langeval *e, const int64_t *hyp, int H, int L, const int64_t *img_idx, void *stream) {
    if (!langeval_valid(e) || H < 0 || L < 1 || L > LMAX) return CAPMI_EINVAL;
    if (H == 0) return 0;
    if (!hyp || !img_idx) return CAPMI_EINVAL;
    hipLaunchKernelGGL(langeval_add_kernel, dim3(H), dim3(CT), 0, (hipStream_t)stream, *e, hyp, H, L, img_idx, log((double)e->n_img));
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_langeval_reduce(const capmi_langeval *e, double *out, int64_t *totals, void *stream) {
    if (!langeval_valid(e) || !out || !totals) return CAPMI_EINVAL;
    hipLaunchKernelGGL(langeval_reduce_kernel, dim3(1), dim3(RT), 0, (hipStream_t)stream, *e, out, totals);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
