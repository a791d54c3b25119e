// Verification ROC (mi355_roc_*): the host side of the all-pairs histogram (its GEMM epilogue, RocArgs, is in rank_common.h, its
// driver roc_pairs_hist in rank.hip), the histogram of given pair scores (utils/roc_curve_from_scratch.py's loop) and the one
// finalize launch: histogram -> tp / fp / fn / tn, rates and the trapezoid AUC.  gfx950 only.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <limits.h>
#include <math.h>

#include <vector>

namespace mi355 {

// Histogram of n given pair scores: class code actual[i] 1 = genuine, 0 = impostor, anything else counts in neither (the
// reference's if/elif chain).  Grid-stride loop, 4 pairs per lane per step when vec; LDS bins u32 [waves or 1][2][T + 1]
// (one sub-histogram per wave when T <= ROC_SUB_T) behind nothing else, then the table (fp32 ceilings, or the float64
// thresholds when F64); flush as the GEMM epilogue does.  Per workgroup fewer than 2^32 pairs (checked on the host).
template <bool F64>
__global__ __launch_bounds__(256) void k_roc_scores(const void* __restrict__ scores, i64 n, const int8_t* __restrict__ actual,
                                                    int vec, RocArgs a) {
    typedef typename std::conditional<F64, double, float>::type V;
    typedef V v4 __attribute__((ext_vector_type(4)));
    typedef int8_t c4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, T = a.T, nb = T + 1;
    const bool sub = T <= ROC_SUB_T;
    const int nbins = (sub ? 4 : 1) * 2 * nb;
    unsigned* bins = reinterpret_cast<unsigned*>(smem);
    V* tab = reinterpret_cast<V*>(smem + ((nbins + 3) & ~3));
    for (int i = tid; i < T; i += 256) tab[i] = F64 ? (V)a.thr[i] : (V)roc_ceil_f32(a.thr[i]);
    for (int i = tid; i < nbins; i += 256) bins[i] = 0u;
    __syncthreads();
    unsigned* mine = bins + (sub ? (tid >> 6) * 2 * nb : 0);
    const V* s = reinterpret_cast<const V*>(scores);
    auto one = [&](V v, int8_t c) {
        if (c == 1 || c == 0) atomicAdd(&mine[(c == 1 ? 0 : nb) + roc_bin(v, tab, a)], 1u);
    };
    const i64 stride = (i64)gridDim.x * 256, n4 = vec ? n / 4 : 0;
    for (i64 i = (i64)blockIdx.x * 256 + tid; i < n4; i += stride) {
        const v4 v = reinterpret_cast<const v4*>(s)[i];
        const c4 c = reinterpret_cast<const c4*>(actual)[i];
        one(v.x, c.x);
        one(v.y, c.y);
        one(v.z, c.z);
        one(v.w, c.w);
    }
    for (i64 i = n4 * 4 + (i64)blockIdx.x * 256 + tid; i < n; i += stride) one(s[i], actual[i]);
    __syncthreads();
    for (int b = tid; b < 2 * nb; b += 256) {
        unsigned long long u = bins[b];
        if (sub) u += (unsigned long long)bins[2 * nb + b] + bins[4 * nb + b] + bins[6 * nb + b];
        if (u) atomicAdd(&a.hist[b], u);
    }
}

// hist [2][T + 1] -> counts [4][T] (tp, fp, fn, tn), totals [2], rates [2][T] (tpr, fpr), auc = |trapezoid(tpr, fpr)|.
// tp[i] = genuine pairs in bins > i (score >= t_i).  One workgroup: each thread owns a contiguous run of bins, walks it down
// from the suffix sum of the runs above; the AUC terms (numpy.trapz's (x[i+1] - x[i]) * (y[i+1] + y[i]) / 2) are summed per
// thread and then over a fixed tree: the same bits every run.
__global__ __launch_bounds__(256) void k_roc_finalize(const i64* __restrict__ hist, int T, i64* __restrict__ counts,
                                                      i64* __restrict__ totals, double* __restrict__ rates, double* __restrict__ auc) {
    __shared__ i64 sg[256], si[256];
    __shared__ double sa[256];
    const int tid = threadIdx.x, nb = T + 1, per = (nb + 255) / 256;
    const int b0 = tid * per < nb ? tid * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    i64 g = 0, m = 0;
    for (int b = b0; b < b1; ++b) { g += hist[b]; m += hist[nb + b]; }
    sg[tid] = g;
    si[tid] = m;
    __syncthreads();
    i64 totg = 0, toti = 0, nextg = 0, nexti = 0;            // totals; the suffix sums of the runs above this one
    for (int t = 0; t < 256; ++t) {
        totg += sg[t];
        toti += si[t];
        if (t > tid) { nextg += sg[t]; nexti += si[t]; }
    }
    double part = 0.0;
    for (int b = b1 - 1; b >= b0; --b) {
        const i64 Sg = hist[b] + nextg, Si = hist[nb + b] + nexti;   // pairs in bins >= b
        if (b >= 1) {
            const int i = b - 1;
            counts[i] = Sg;
            counts[T + i] = Si;
            counts[2 * T + i] = totg - Sg;
            counts[3 * T + i] = toti - Si;
            const double tpr = (double)Sg / (double)totg, fpr = (double)Si / (double)toti;   // 0 / 0 = NaN
            rates[i] = tpr;
            rates[T + i] = fpr;
            if (b < T) {                                       // the segment (i, i + 1)
                const double tpr1 = (double)nextg / (double)totg, fpr1 = (double)nexti / (double)toti;
                part += (fpr1 - fpr) * (tpr1 + tpr) / 2.0;
            }
        }
        nextg = Sg;
        nexti = Si;
    }
    sa[tid] = part;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sa[tid] += sa[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        auc[0] = fabs(sa[0]);
        totals[0] = totg;
        totals[1] = toti;
    }
}

int roc_check_thresholds(const double* thr, int T, const char* who, RocArgs* a) {
    MI355_REQUIRE(thr, "%s: null thresholds (host pointer)", who);
    MI355_REQUIRE(T >= 1 && T <= ROC_MAX_T, "%s: T=%d thresholds outside [1, %d]", who, T, ROC_MAX_T);
    for (int i = 0; i < T; ++i) {
        MI355_REQUIRE(isfinite(thr[i]), "%s: threshold %d is not finite (%g)", who, i, thr[i]);
        MI355_REQUIRE(i == 0 || thr[i] >= thr[i - 1], "%s: thresholds must be ascending: t[%d] = %.17g < t[%d] = %.17g", who, i,
                      thr[i], i - 1, thr[i - 1]);
    }
    if (!a) return OK;
    a->T = T;
    a->top = 1;
    while (a->top * 2 <= T) a->top *= 2;
    // a grid whose fp32 ceilings stay within one step of the straight line through the ends: guess, then fix
    std::vector<double> f(T);
    for (int i = 0; i < T; ++i) f[i] = roc_ceil_f32(thr[i]);
    a->uniform = 0;
    a->scale = 0.f;
    if (T >= 2 && f[T - 1] > f[0]) {
        const double h = (f[T - 1] - f[0]) / (T - 1);
        bool ok = true;
        for (int i = 0; i < T && ok; ++i) ok = fabs(f[i] - (f[0] + i * h)) <= h;
        if (ok) {
            a->uniform = 1;
            a->scale = (float)(1.0 / h);
        }
    }
    return OK;
}

int roc_check_pairs(const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude, int64_t idx_offset,
                    const double* thresholds_dev, int64_t* hist, const char* who, RocArgs* a) {
    MI355_REQUIRE(query_labels && gallery_labels, "%s: null query_labels/gallery_labels", who);
    MI355_REQUIRE(thresholds_dev, "%s: null thresholds_dev", who);
    MI355_REQUIRE(hist, "%s: null hist", who);
    a->qlab = (const i64*)query_labels;
    a->glab = (const i64*)gallery_labels;
    a->excl = (const i64*)exclude;
    a->idx_offset = idx_offset;
    a->thr = thresholds_dev;
    a->hist = (unsigned long long*)hist;
    return OK;
}

RocArgs roc_from(const RocArgs& a, i64 q0) {
    RocArgs r = a;
    r.qlab += q0;
    if (r.excl) r.excl += q0;
    return r;
}

i64 roc_query_block(i64 Q, i64 G) {
    // the split planes of one call stay those of mi355_cosine_scores (256 * 64 queries); the 1-D grid stays < 2^31
    i64 qb = Q < 256 * 64 ? Q : 256 * 64;
    while (qb > 128 && (i64)cdiv(G, RK_BN) * cdiv(qb, 64) >= INT_MAX) qb /= 2;
    return qb;
}

// LDS of k_roc_scores: the bins, then the table
static size_t roc_scores_lds(int T, int f64) {
    const size_t bins = (size_t)(T <= ROC_SUB_T ? 4 : 1) * 2 * (T + 1);
    return align_up(bins * sizeof(unsigned), 16) + (size_t)T * (f64 ? sizeof(double) : sizeof(float));
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_roc_scores_hist(const void* scores, int scores_f64, int64_t n, const int8_t* actual, const double* thresholds,
                          const double* thresholds_dev, int T, int64_t* hist, void* stream) {
    const char* who = "roc_scores_hist";
    RocArgs a{};
    if (int e = roc_check_thresholds(thresholds, T, who, &a)) return e;
    MI355_REQUIRE(thresholds_dev && hist, "%s: null thresholds_dev/hist", who);
    MI355_REQUIRE(n >= 0 && n <= ((int64_t)1 << 40), "%s: bad length n=%lld", who, (long long)n);
    MI355_REQUIRE(n == 0 || (scores && actual), "%s: null scores/actual", who);
    MI355_REQUIRE(scores_f64 == 0 || scores_f64 == 1, "%s: scores_f64 must be 0 or 1, got %d", who, scores_f64);
    a.thr = thresholds_dev;
    a.hist = (unsigned long long*)hist;
    hipStream_t st = (hipStream_t)stream;
    MI355_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)2 * (T + 1) * sizeof(int64_t), st));
    if (n == 0) return OK;
    const size_t lds = roc_scores_lds(T, scores_f64);
    const int vec = (((uintptr_t)scores & (scores_f64 ? 31 : 15)) == 0) && (((uintptr_t)actual & 3) == 0);
    int slots = 0;
    static int cache32[MI355_MAX_DEVICES] = {0}, cache64[MI355_MAX_DEVICES] = {0};
    const void* fn = scores_f64 ? (const void*)k_roc_scores<true> : (const void*)k_roc_scores<false>;
    // (the kernel's LDS limit is set once per device: to its largest request, over every T)
    const size_t lds_max = roc_scores_lds(ROC_SUB_T, scores_f64) > roc_scores_lds(ROC_MAX_T, scores_f64)
                               ? roc_scores_lds(ROC_SUB_T, scores_f64) : roc_scores_lds(ROC_MAX_T, scores_f64);
    if (int e = kernel_slots(fn, lds_max, scores_f64 ? cache64 : cache32, &slots)) return e;
    const i64 want = cdiv(n, 256 * 16);
    const int blocks = (int)(want < slots ? want : slots);
    MI355_REQUIRE(n / blocks < ((int64_t)1 << 32) - 1, "%s: n=%lld too large for %d workgroups", who, (long long)n, blocks);
    if (scores_f64)
        hipLaunchKernelGGL((k_roc_scores<true>), dim3(blocks), dim3(256), lds, st, scores, (i64)n, actual, vec, a);
    else
        hipLaunchKernelGGL((k_roc_scores<false>), dim3(blocks), dim3(256), lds, st, scores, (i64)n, actual, vec, a);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_roc_finalize(const int64_t* hist, int T, int64_t* counts, int64_t* totals, double* rates, double* auc, void* stream) {
    MI355_REQUIRE(hist && counts && totals && rates && auc, "roc_finalize: null pointer");
    MI355_REQUIRE(T >= 1 && T <= ROC_MAX_T, "roc_finalize: T=%d thresholds outside [1, %d]", T, ROC_MAX_T);
    hipLaunchKernelGGL(k_roc_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, (const i64*)hist, T, (i64*)counts,
                       (i64*)totals, rates, auc);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
