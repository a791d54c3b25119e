// Score normalisation: CSLS (Conneau et al., ICLR 2018) and cohort normalisation (Z-, T-, S- and adaptive S-norm) as one affine
// map of the cosine score, t = s * (aq[q] + ag[g]) - (bq[q] + bg[g]).  include/mi355_retrieval.h states the map bit for bit.
//   the map itself ......... lives in the cosine GEMM's epilogues (rank_common.h): AdjSelectEpi<FK, FILT> writes the
//                            adjusted scores into the transposed LDS tile that the fused per-tile selection reads (k <= 8, Q > 4:
//                            no Q x G slab, no LDS beyond the unadjusted selection's), AdjSlabEpi writes the adjusted slab (every
//                            other shape, and mi355_cosine_scores_adjusted).  The block loop is adjusted_search (rank.hip), the
//                            fp16 rows' entries are in rank_f16.hip beside their siblings.
//   mi355_topn_stats ....... count, mean and population deviation of each row of a top-n result, and the coefficients a cohort
//                            normalisation makes of them.  One thread per row: the sums run in float64 in slot order (the order
//                            is part of the result), two passes over at most 1024 slots that the first pass left in L1 / L2.
//                            Rows are independent; there are no atomics and no host sync.
// This file holds the statistics kernel, the argument checks every adjusted entry shares and the fp32 rows' entries.  gfx950 only.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

__global__ __launch_bounds__(256) void k_topn_stats(const float* __restrict__ val, const i64* __restrict__ idx, i64 N, int n,
                                                    double half, double min_std, float* __restrict__ mean, float* __restrict__ sd,
                                                    int* __restrict__ count, float* __restrict__ a, float* __restrict__ b) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const float* v = val + r * n;
    const i64* ix = idx + r * n;
    int cnt = 0;
    double sum = 0.0;
    for (int j = 0; j < n; ++j)
        if (ix[j] >= 0) { sum += (double)v[j]; ++cnt; }
    double m = 0.0, s = 0.0;
    if (cnt > 0) {
        m = sum / (double)cnt;
        double ss = 0.0;
        for (int j = 0; j < n; ++j)
            if (ix[j] >= 0) {
                const double d = (double)v[j] - m;
                double sq = d * d;
                asm volatile("" : "+v"(sq));            // the rounded square in registers: the float64 model adds rounded squares
                ss += sq;
            }
        s = sqrt(ss / (double)cnt);
    }
    mean[r] = (float)m;
    sd[r] = (float)s;
    count[r] = cnt;
    if (a) {
        const double sf = s > min_std ? s : min_std;    // (a NaN deviation comes with a NaN mean: b is NaN then)
        a[r] = (float)(half / sf);
        b[r] = (float)((m * half) / sf);
    }
}

int adjust_check(const void* queries, i64 Q, const GalleryRows& g, i64 G, int dim, int k, bool topk, const mi355_score_adjust* adjust,
                 const mi355_rank_filter* filter, i64 idx_offset, i64 query_block, const void* out_val, const void* out_idx,
                 const char* who, ScoreAdjust* adj, RankFilter* f) {
    MI355_REQUIRE(queries && g.rows(), "%s: null queries/gallery pointer", who);
    MI355_REQUIRE(adjust, "%s: null adjust (use the unadjusted entry)", who);
    MI355_REQUIRE(out_val && (out_idx || !topk), "%s: null output", who);
    MI355_REQUIRE(adjust->aq || adjust->ag, "%s: aq and ag are both null (the score's factor would be 0 everywhere)", who);
    MI355_REQUIRE(Q >= 0 && G >= 1 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    MI355_REQUIRE(Q <= INT_MAX && G < ((int64_t)1 << 31) - RK_BN, "%s: shape too large Q=%lld G=%lld", who, (long long)Q,
                  (long long)G);
    if (topk) {
        MI355_REQUIRE(k >= 1 && k <= LARGE_K, "%s: k=%d outside [1,%d]", who, k, LARGE_K);
        MI355_REQUIRE(k <= G, "%s: k=%d exceeds gallery rows %lld", who, k, (long long)G);
    }
    MI355_REQUIRE(query_block >= 0, "%s: query_block=%lld must be >= 0 (0: the default rule)", who, (long long)query_block);
    MI355_REQUIRE(((uintptr_t)g.f16 & 15) == 0, "%s: gallery buffer must be 16-byte aligned", who);
    *adj = ScoreAdjust{adjust->aq, adjust->bq, adjust->ag, adjust->bg};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, f)) return e;
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_rank_adjusted_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || G < 1 || dim < 1 || k < 0 || k > LARGE_K) return 0;
    return carve(nullptr, Q, G, dim, k, f32_rows(nullptr, 0).planes_bytes, true, k > 0).total;
}

int mi355_rank_topk_adjusted(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                             int k, float eps, int64_t idx_offset, const mi355_score_adjust* adjust, const mi355_rank_filter* filter,
                             int64_t query_block, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                             void* stream) {
    const GalleryRows g = f32_rows(gallery, gallery_is_normalized);
    ScoreAdjust adj{};
    RankFilter f{};
    if (int e = adjust_check(queries, Q, g, G, dim, k, true, adjust, filter, idx_offset, query_block, out_val, out_idx,
                             "rank_topk_adjusted", &adj, &f))
        return e;
    if (Q == 0) return OK;
    return adjusted_search(queries, Q, g, G, dim, eps, k, idx_offset, adj, filter ? &f : nullptr, query_block, out_val, (i64*)out_idx,
                           workspace, workspace_bytes, (hipStream_t)stream, "rank_topk_adjusted");
}

int mi355_cosine_scores_adjusted(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                                 float eps, const mi355_score_adjust* adjust, int64_t query_block, float* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    const GalleryRows g = f32_rows(gallery, gallery_is_normalized);
    ScoreAdjust adj{};
    if (int e = adjust_check(queries, Q, g, G, dim, 0, false, adjust, nullptr, 0, query_block, out, nullptr, "cosine_scores_adjusted",
                             &adj, nullptr))
        return e;
    if (Q == 0) return OK;
    return adjusted_search(queries, Q, g, G, dim, eps, 0, 0, adj, nullptr, query_block, out, nullptr, workspace, workspace_bytes,
                           (hipStream_t)stream, "cosine_scores_adjusted");
}

int mi355_topn_stats(const float* val, const int64_t* idx, int64_t N, int n, double half, double min_std, float* mean, float* std,
                     int32_t* count, float* a, float* b, void* stream) {
    MI355_REQUIRE(val && idx && mean && std && count, "topn_stats: null pointer");
    MI355_REQUIRE((a != nullptr) == (b != nullptr), "topn_stats: a and b go together (one of them is null)");
    MI355_REQUIRE(N >= 0 && N <= INT_MAX, "topn_stats: N=%lld outside [0, 2^31)", (long long)N);
    MI355_REQUIRE(n >= 1 && n <= LARGE_K, "topn_stats: n=%d outside [1,%d]", n, LARGE_K);
    MI355_REQUIRE(isfinite(half) && isfinite(min_std) && min_std >= 0.0, "topn_stats: half=%g and min_std=%g must be finite, min_std >= 0",
                  half, min_std);
    if (N == 0) return OK;
    hipLaunchKernelGGL(k_topn_stats, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, val, (const i64*)idx, (i64)N, n,
                       half, min_std, mean, std, count, a, b);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
