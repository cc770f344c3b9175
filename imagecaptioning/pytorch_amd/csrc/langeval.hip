// Corpus CIDEr, BLEU-1..4 and ROUGE-L on the GPU (gfx950): the Java-free metrics of coco-caption over token ids, for the
// validation pass that picks model-best.pth during SCST (eval_utils.language_eval -> lang_stats; formulas in include/capmi.h).
//
// Three kinds of launch.  Building (once per split): a workgroup per image inserts the image's distinct reference n-grams into an
// open-addressing table in HBM (atomicCAS on the key, atomicAdd on the count), then a workgroup per reference stores the four
// tf-idf norms, so that scoring never looks a reference n-gram up.  Adding (once per decoded batch): a workgroup per hypothesis
// row cooks the row in LDS -- one lane per (order, start position), ngram_metrics.h -- and walks the image's references once:
// the occurrences of each hypothesis n-gram in the reference feed the CIDEr dot product and BLEU's clip count together; then one
// wave per reference runs the LCS rows of ROUGE-L in registers (a row of the table is a prefix maximum across the lanes).
// Reducing: one workgroup sums the per-image integers as integers and the scores in a fixed order.
//
// All of it is latency bound (a few hundred hash probes and LDS compares per caption): the point is that the decoded rows never
// leave HBM and the host reads eight doubles per evaluation.
//
// Cooking, staging, the token convention (EvalTokens) and the idf rule (CorpusIdf) are the family's (ngram_metrics.h); this file
// keeps the document-frequency build, ROUGE-L, the walks' per-pair logic and the reductions.
#include "ngram_metrics.h"

using namespace capmi;

namespace {

constexpr double BETA = 1.2;

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
    __shared__ Row Cur, Old;
    const EvalTokens tokens{e.err};
    const int r0 = e.ref_off[blockIdx.x], r1 = e.ref_off[blockIdx.x + 1];
    for (int r = r0; r < r1; ++r) {
        Lane c = cook_row(Cur, e.refs + (size_t)r * e.ref_w, e.ref_w, tokens);
        for (int o = r0; o < r; ++o) {                       // the image's earlier references
            stage_keys(Old, e.refs + (size_t)o * e.ref_w, e.ref_w, tokens);
            if (c.first && Old.count(c.k(), c.key)) c.first = false;
            __syncthreads();
        }
        if (c.first) df_insert(e.table_keys, e.table_counts, e.table_cap, c.key, e.err);
        __syncthreads();
    }
}

__device__ __forceinline__ CorpusIdf idf_of(const capmi_langeval &e, double log_n) {
    return CorpusIdf{e.table_keys, e.table_counts, e.table_cap, e.n_img, log_n};
}

// One workgroup per reference: ref_norm [total_refs, 4].
__global__ __launch_bounds__(CT) void langeval_ref_norm_kernel(capmi_langeval e, double log_n) {
    const int r = blockIdx.x;
    row_norms(e.refs + (size_t)r * e.ref_w, e.ref_w, EvalTokens{e.err}, idf_of(e, log_n), e.ref_norm + (size_t)r * NG);
}

// The entry of position g of img_idx [G] counts when no later entry names the same image and the image is inside the split.
// Every thread of the workgroup calls it.
__device__ __forceinline__ bool entry_counts(const int64_t *__restrict__ img_idx, int G, int g, int n_img, int32_t *err, int *img) {
    const int64_t img64 = img_idx[g];
    int later = 0;
    for (int j = g + 1 + threadIdx.x; j < G; j += blockDim.x) later |= img_idx[j] == img64;
    if (__syncthreads_or(later)) return false;
    if (img64 < 0 || img64 >= n_img) {
        if (threadIdx.x == 0) atomicOr(err, CAPMI_LANGEVAL_E_IMAGE);
        return false;
    }
    *img = (int)img64;
    return true;
}

// One workgroup scores one row against the references of image img: cider / rouge / bleu_stats / lens [oi], lcs [reference]
// (skipped when NULL).  oi is the image for capmi_langeval_add and (image, slot) for the oracle scores of capmi_diveval_add.
__device__ __forceinline__ void score_row(const capmi_langeval &e, const int64_t *__restrict__ row, int L, int img, size_t oi,
                                          int32_t *__restrict__ lcs_out, double log_n) {
    __shared__ Row Hr, Rr;
    __shared__ double contrib[CT], norm_h[NG], score[NG], wave_p[NG], wave_r[NG];
    __shared__ int icontrib[CT];
    const EvalTokens tokens{e.err};
    const int tid = threadIdx.x;
    const int r0 = e.ref_off[img], r1 = e.ref_off[img + 1];

    // ---- the hypothesis: distinct n-grams, their counts and tf-idf weights
    const Lane c = cook_row(Hr, row, L, tokens);
    const int len_h = Hr.len;
    const double idf = c.first ? idf_of(e, log_n)(c.key) : 0.0;
    const double vh = (double)c.tf * idf;
    contrib[tid] = c.first ? vh : 0.0;
    __syncthreads();
    if (tid < NG) {
        norm_h[tid] = order_norm(contrib, tid);
        score[tid] = 0.0;
    }

    // ---- one walk over the references: CIDEr dot products, BLEU clip counts, the closest length
    int max_tf = 0;
    ClosestLen closest;
    for (int r = r0; r < r1; ++r) {
        __syncthreads();                                     // contrib / Rr of the previous reference are consumed
        stage_keys(Rr, e.refs + (size_t)r * e.ref_w, e.ref_w, tokens);
        const int tf_r = c.first ? Rr.count(c.k(), c.key) : 0;
        max_tf = max(max_tf, tf_r);
        contrib[tid] = c.first ? vh * ((double)tf_r * idf) : 0.0;     // the reference's weight of the same n-gram: same idf
        __syncthreads();
        if (tid < NG) score[tid] += order_cosine(order_dot(contrib, tid), norm_h[tid], e.ref_norm[(size_t)r * NG + tid]);
        closest.see(Rr.len, len_h);
    }
    const int best_l = closest.len;
    const int correct = clipped_matches(icontrib, c.first, c.tf, max_tf);
    if (tid < NG) {
        e.bleu_stats[(oi * NG + tid) * 2 + 0] = max(0, len_h - tid);
        e.bleu_stats[(oi * NG + tid) * 2 + 1] = correct;
    }
    if (tid == 0) {
        double m = 0.0;
        for (int q = 0; q < NG; ++q) m += score[q];
        e.cider[oi] = r1 > r0 ? m / NG / (double)(r1 - r0) * 10.0 : 0.0;
        e.lens[oi * 2 + 0] = len_h;
        e.lens[oi * 2 + 1] = best_l;
    }

    // ---- ROUGE-L: wave w takes references w, w + 4, ...; lane j holds column j + 1 of the LCS table's current row.
    // With x[j] = row[i-1][j-1] + 1 where the tokens match and row[i-1][j] elsewhere, row[i] is the prefix maximum of x.
    const int wave = tid / CAPMI_WAVE, lane = tid % CAPMI_WAVE;
    const int th = lane < len_h ? Hr.tok[lane] : -1;
    double p_max = 0.0, r_max = 0.0;
    for (int r = r0 + wave; r < r1; r += NG) {
        const int tr = tokens.load(e.refs + (size_t)r * e.ref_w, e.ref_w, lane);
        const int len_r = caption_len<EvalTokens::KEEP_EOS>(tr, e.ref_w, lane);
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
        if (lane == 0 && lcs_out) lcs_out[r] = lcs;
        if (len_h > 0) p_max = fmax(p_max, (double)lcs / (double)len_h);
        if (len_r > 0) r_max = fmax(r_max, (double)lcs / (double)len_r);
    }
    if (lane == 0) { wave_p[wave] = p_max; wave_r[wave] = r_max; }
    __syncthreads();
    if (tid == 0) {
        double p = 0.0, q = 0.0;
        for (int w = 0; w < NG; ++w) { p = fmax(p, wave_p[w]); q = fmax(q, wave_r[w]); }
        e.rouge[oi] = (p != 0.0 && q != 0.0) ? (1.0 + BETA * BETA) * p * q / (q + BETA * BETA * p) : 0.0;
    }
}

// One workgroup per hypothesis row; a later row of the call that describes the same image counts.
__global__ __launch_bounds__(CT) void langeval_add_kernel(capmi_langeval e, const int64_t *__restrict__ hyp, int H, int L,
                                                         const int64_t *__restrict__ img_idx, double log_n) {
    int img;
    if (!entry_counts(img_idx, H, blockIdx.x, e.n_img, e.err, &img)) return;
    score_row(e, hyp + (size_t)blockIdx.x * L, L, img, (size_t)img, e.lcs, log_n);
    if (threadIdx.x == 0) e.seen[img] = 1;
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
        bleu_of_counts(ti, out);
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
    return table_cap_ok(e->table_cap);
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

// ---------------------------------------------------------------------------------------------------------------------------
// Diversity of n sampled captions per image (eval_multi: Div-n, mBLEU, self-CIDEr, oracle scores; formulas in include/capmi.h).
// The same cooking and the same walk as above with the image's other sampled captions in the place of its references, then one
// small symmetric eigenproblem per image.  Rows g*n .. g*n+n-1 of hyp are group g, the captions of image img_idx[g].
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int NO = 6;                       // oracle scores per slot: CIDEr, Bleu_1..4, ROUGE_L
constexpr int ET = CAPMI_WAVE;              // one wave per image solves the eigenproblem

// One workgroup per caption: norm [img, slot, 4], as langeval_ref_norm_kernel does for a reference.
__global__ __launch_bounds__(CT) void diveval_norm_kernel(capmi_diveval d, const int64_t *__restrict__ hyp, int B, int L,
                                                         const int64_t *__restrict__ img_idx, double log_n) {
    const int g = blockIdx.x / d.n, s = blockIdx.x % d.n;
    int img;
    if (!entry_counts(img_idx, B, g, d.lang.n_img, d.err, &img)) return;
    row_norms(hyp + (size_t)blockIdx.x * L, L, EvalTokens{d.err}, idf_of(d.lang, log_n), d.norm + ((size_t)img * d.n + s) * NG);
}

// One workgroup per caption (image, slot s) walks the n captions of its image once.  Slot o >= s: K[s][o] and its mirror.
// Slot o != s: the clip counts and the closest length of mBLEU with the other captions as references.  Slot o < s: an n-gram
// that o holds is not first seen in s.
__global__ __launch_bounds__(CT) void diveval_walk_kernel(capmi_diveval d, const int64_t *__restrict__ hyp, int B, int L,
                                                         const int64_t *__restrict__ img_idx, double log_n) {
    __shared__ Row Hr, Rr;
    __shared__ int icontrib[CT], correct_s[NG];
    __shared__ double contrib[CT], cos_s[NG];
    const EvalTokens tokens{d.err};
    const int n = d.n, tid = threadIdx.x, g = blockIdx.x / n, s = blockIdx.x % n;
    int img;
    if (!entry_counts(img_idx, B, g, d.lang.n_img, d.err, &img)) return;
    const int64_t *rows = hyp + (size_t)g * n * L;

    const Lane c = cook_row(Hr, rows + (size_t)s * L, L, tokens);
    const int len_h = Hr.len;
    const double idf = c.first ? idf_of(d.lang, log_n)(c.key) : 0.0;
    const double vh = (double)c.tf * idf;
    if (c.k() == 0 && c.first) atomicOr(d.vocab_bits + (Hr.tok[c.i()] >> 5), 1u << (Hr.tok[c.i()] & 31));      // ids < 65535: inside the bitmap

    const double *norm = d.norm + (size_t)img * n * NG;
    double *K = d.K + (size_t)img * n * n;
    bool first_in_image = c.first;
    int max_tf = 0;
    ClosestLen closest;
    for (int o = 0; o < n; ++o) {
        __syncthreads();                                     // Rr / contrib / cos_s of the previous caption are consumed
        stage_keys(Rr, rows + (size_t)o * L, L, tokens);
        const int tf_r = c.first ? Rr.count(c.k(), c.key) : 0;
        if (o != s) {
            max_tf = max(max_tf, tf_r);
            closest.see(Rr.len, len_h);
            if (o < s && tf_r) first_in_image = false;
        }
        if (o >= s) {
            contrib[tid] = c.first ? vh * ((double)tf_r * idf) : 0.0;
            __syncthreads();
            if (tid < NG) cos_s[tid] = order_cosine(order_dot(contrib, tid), norm[s * NG + tid], norm[o * NG + tid]);
            __syncthreads();
            if (tid == 0) {
                double m = 0.0;
                for (int q = 0; q < NG; ++q) m += cos_s[q];
                const double v = m / NG * 10.0;
                K[(size_t)s * n + o] = v;
                K[(size_t)o * n + s] = v;
            }
        }
    }
    const int correct = clipped_matches(icontrib, c.first, c.tf, max_tf);
    if (tid < NG) correct_s[tid] = correct;
    __syncthreads();
    icontrib[tid] = first_in_image;
    __syncthreads();
    if (tid < 2) {
        int cnt = 0;
        for (int j = 0; j < LMAX; ++j) cnt += icontrib[tid * LMAX + j];
        d.slot_distinct[((size_t)img * n + s) * 2 + tid] = cnt;
    }
    if (tid == 0) {
        int32_t *st = d.mbleu_stats + ((size_t)img * n + s) * 10;
        int cnt[10];
        bleu_counts(cnt, len_h, correct_s, 1, closest.len);
        for (int q = 0; q < 10; ++q) st[q] = cnt[q];
        double b[NG];
        bleu_of_counts(cnt, b);
        d.sent_bleu2[(size_t)img * n + s] = b[1];
    }
}

// One workgroup per caption against the image's references; e is d.lang with its outputs indexed by (image, slot).
__global__ __launch_bounds__(CT) void diveval_oracle_kernel(capmi_langeval e, int n, const int64_t *__restrict__ hyp, int B, int L,
                                                           const int64_t *__restrict__ img_idx, double log_n) {
    int img;
    if (!entry_counts(img_idx, B, blockIdx.x / n, e.n_img, e.err, &img)) return;
    score_row(e, hyp + (size_t)blockIdx.x * L, L, img, (size_t)img * n + blockIdx.x % n, nullptr, log_n);
}

// One wave per image: the eigenvalues of K/10 by cyclic Jacobi in LDS (ngram_metrics.h), self_cider, and the image's sums over
// its slots.
__global__ __launch_bounds__(ET) void diveval_finish_kernel(capmi_diveval d, int B, const int64_t *__restrict__ img_idx) {
    __shared__ double A[NMAX][NMAX + 1], ev[NMAX];
    const int n = d.n, lane = threadIdx.x;
    int img;
    if (!entry_counts(img_idx, B, blockIdx.x, d.lang.n_img, d.err, &img)) return;
    const double *K = d.K + (size_t)img * n * n;
    for (int idx = lane; idx < n * n; idx += ET) A[idx / n][idx % n] = K[idx] / 10.0;
    __syncthreads();
    jacobi_eigenvalues(A, n, lane, ev, CAPMI_DIVEVAL_SWEEPS);
    if (lane < n) d.eig[(size_t)img * n + lane] = ev[lane];
    if (lane == 0) {
        d.self_cider[img] = self_cider_of(ev, n);            // every caption empty: 0, not NaN
        d.seen[img] = 1;
    }
    if (lane < 3) {                                          // distinct 1-grams, distinct 2-grams, tokens
        int total = 0;
        for (int s = 0; s < n; ++s)
            total += lane < 2 ? d.slot_distinct[((size_t)img * n + s) * 2 + lane] : d.mbleu_stats[((size_t)img * n + s) * 10 + 8];
        if (lane < 2) d.distinct[(size_t)img * 2 + lane] = total;
        else d.tokens[img] = total;
    }
    if (d.oracle && lane < n) {
        const size_t oi = (size_t)img * n + lane;
        int cnt[10];
        bleu_counts(cnt, d.lang.lens[oi * 2 + 0], d.lang.bleu_stats + oi * NG * 2 + 1, 2, d.lang.lens[oi * 2 + 1]);
        double b[NG];
        bleu_of_counts(cnt, b);
        double *o = d.oracle_scores + oi * NO;
        o[0] = d.lang.cider[oi];
        for (int q = 0; q < NG; ++q) o[1 + q] = b[q];
        o[5] = d.lang.rouge[oi];
    }
}

constexpr int NF = 3 + 2 * NO;   // float sums: Div1, Div2, self_cider, oracle max x 6, oracle mean x 6

// One workgroup.  Integers (the per-slot BLEU counts, the bitmap's popcount, the images) are added with LDS integer atomics; every
// thread sums the floats of its images (stride RT), then one thread per quantity adds the RT partial sums in index order.
__global__ __launch_bounds__(RT) void diveval_reduce_kernel(capmi_diveval d, double *__restrict__ out, int64_t *__restrict__ totals) {
    __shared__ unsigned long long ti[NMAX * 10], n_seen, n_words;
    __shared__ double sd[NF][RT], td[NF];
    const int tid = threadIdx.x, n = d.n, per = n * 10;
    for (int q = tid; q < per; q += RT) ti[q] = 0;
    if (tid == 0) { n_seen = 0; n_words = 0; }
    __syncthreads();
    for (size_t idx = tid; idx < (size_t)d.lang.n_img * per; idx += RT)
        if (d.seen[idx / per]) atomicAdd(&ti[idx % per], (unsigned long long)d.mbleu_stats[idx]);
    int bits = 0;
    for (int w = tid; w < CAPMI_DIVEVAL_VOCAB_WORDS; w += RT) bits += __popc(d.vocab_bits[w]);
    atomicAdd(&n_words, (unsigned long long)bits);
    double acc[NF] = {};
    int mine = 0;
    for (int img = tid; img < d.lang.n_img; img += RT) {
        if (!d.seen[img]) continue;
        ++mine;
        const double tokens = 1e-6 + (double)d.tokens[img];
        acc[0] += (double)d.distinct[(size_t)img * 2 + 0] / tokens;
        acc[1] += (double)d.distinct[(size_t)img * 2 + 1] / tokens;
        acc[2] += d.self_cider[img];
        if (d.oracle)
            for (int x = 0; x < NO; ++x) {
                const double *o = d.oracle_scores + (size_t)img * n * NO + x;
                double best = o[0], sum = o[0];
                for (int s = 1; s < n; ++s) { best = fmax(best, o[(size_t)s * NO]); sum += o[(size_t)s * NO]; }
                acc[3 + x] += best;
                acc[3 + NO + x] += sum / (double)n;
            }
    }
    atomicAdd(&n_seen, (unsigned long long)mine);
    for (int q = 0; q < NF; ++q) sd[q][tid] = acc[q];
    __syncthreads();
    if (tid < NF) {
        double sum = 0.0;
        for (int j = 0; j < RT; ++j) sum += sd[tid][j];
        td[tid] = sum;
    }
    for (int q = tid; q < per; q += RT) totals[q] = (int64_t)ti[q];
    __syncthreads();
    if (tid == 0) {
        const double cnt = (double)n_seen;
        double mb[NG] = {};
        for (int s = 0; s < n; ++s) {                        // the corpus Bleu of slot s, then the mean over the slots
            double b[NG];
            bleu_of_counts(&ti[s * 10], b);
            for (int q = 0; q < NG; ++q) mb[q] += b[q];
        }
        out[0] = cnt > 0 ? td[0] / cnt : 0.0;
        out[1] = cnt > 0 ? td[1] / cnt : 0.0;
        out[2] = (double)n_words;
        for (int q = 0; q < NG; ++q) out[3 + q] = cnt > 0 ? mb[q] / (double)n : 0.0;
        out[7] = cnt > 0 ? td[2] / cnt : 0.0;
        out[8] = cnt;
        out[9] = (double)*d.err;
        for (int x = 0; x < 2 * NO; ++x) out[10 + x] = (d.oracle && cnt > 0) ? td[3 + x] / cnt : 0.0;
    }
}
static_assert(10 + 2 * NO == CAPMI_DIVEVAL_NOUT, "out [CAPMI_DIVEVAL_NOUT]");

bool diveval_valid(const capmi_diveval *d) {
    if (!d) return false;
    const capmi_langeval &e = d->lang;
    if (!e.table_keys || !e.table_counts || e.n_img < 1 || !table_cap_ok(e.table_cap)) return false;
    if (d->n < 2 || d->n > NMAX) return false;
    if (!d->norm || !d->slot_distinct || !d->distinct || !d->tokens || !d->mbleu_stats || !d->sent_bleu2 || !d->K || !d->eig ||
        !d->self_cider || !d->seen || !d->err || !d->vocab_bits || e.err != d->err)
        return false;
    if (d->oracle && (!d->oracle_scores || !e.refs || !e.ref_off || !e.ref_norm || !e.cider || !e.rouge || !e.bleu_stats || !e.lens ||
                      e.total_refs < 0 || e.ref_w < 1 || e.ref_w > LMAX))
        return false;
    return true;
}

}  // namespace

extern "C" int capmi_diveval_add(const capmi_diveval *d, const int64_t *hyp, int B, int L, const int64_t *img_idx, void *stream) {
    if (!diveval_valid(d) || B < 0 || L < 1 || L > LMAX) return CAPMI_EINVAL;
    if (B == 0) return 0;
    if (!hyp || !img_idx) return CAPMI_EINVAL;
    const double log_n = log((double)d->lang.n_img);
    hipLaunchKernelGGL(diveval_norm_kernel, dim3(B * d->n), dim3(CT), 0, (hipStream_t)stream, *d, hyp, B, L, img_idx, log_n);
    CAPMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(diveval_walk_kernel, dim3(B * d->n), dim3(CT), 0, (hipStream_t)stream, *d, hyp, B, L, img_idx, log_n);
    CAPMI_CHECK_LAUNCH();
    if (d->oracle) {
        hipLaunchKernelGGL(diveval_oracle_kernel, dim3(B * d->n), dim3(CT), 0, (hipStream_t)stream, d->lang, d->n, hyp, B, L, img_idx,
                           log_n);
        CAPMI_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(diveval_finish_kernel, dim3(B), dim3(ET), 0, (hipStream_t)stream, *d, B, img_idx);
    CAPMI_CHECK_LAUNCH();
    return 0;
}

extern "C" int capmi_diveval_reduce(const capmi_diveval *d, double *out, int64_t *totals, void *stream) {
    if (!diveval_valid(d) || !out || !totals) return CAPMI_EINVAL;
    hipLaunchKernelGGL(diveval_reduce_kernel, dim3(1), dim3(RT), 0, (hipStream_t)stream, *d, out, totals);
    CAPMI_CHECK_LAUNCH();
    return 0;
}
