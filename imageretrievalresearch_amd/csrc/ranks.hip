// Full-gallery ranks of every positive (mi355_rank_positives*): the host side shared by the fp32 and fp16 counting passes (their
// GEMM epilogue, RanksArgs, is in rank_common.h, their driver rank_positives in rank.hip), the composites of the positives and the
// finalize launch: counts -> ranks, average precision and first rank per query.  gfx950 only.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <limits.h>

namespace mi355 {

// (global row, score) of a positive -> its composite: score_key in the high word, ~local row in the low one
__global__ __launch_bounds__(256) void k_ranks_keys(const i64* __restrict__ indices, const float* __restrict__ scores, i64 nnz,
                                                    i64 idx_offset, unsigned long long* __restrict__ keys) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nnz; i += stride)
        keys[i] = rank_composite(score_key(scores[i]), (unsigned)(indices[i] - idx_offset));
}

// One wave per query: the inclusive prefix sum of before[] over the query's segment, 64 positives at a time with the prefix
// carried; rank(p_i) = i + 1 + sum_{b <= i} before[b].  AP = (sum_i (i + 1) / rank(p_i)) / R_q in float64, the terms added in
// the order i = 0, 1, 2, .. (every lane adds the chunk's 64 terms in lane order): the same bits as a sequential host loop.
// A query without positives gets AP 0 and first rank 0.
__global__ __launch_bounds__(256) void k_ranks_finalize(const i64* __restrict__ offsets, const unsigned* __restrict__ before, i64 Q,
                                                        i64* __restrict__ ranks, double* __restrict__ ap, i64* __restrict__ first) {
    const int lane = threadIdx.x & 63;
    const i64 q = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const i64 s0 = offsets[q], R = offsets[q + 1] - s0;
    i64 carry = 0, fr = 0;
    double sum = 0.0;
    for (i64 c0 = 0; c0 < R; c0 += 64) {
        const i64 i = c0 + lane;
        i64 incl = i < R ? (i64)before[s0 + i] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const i64 v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        const i64 rank = i + 1 + carry + incl;
        double term = 0.0;
        if (i < R) {
            ranks[s0 + i] = rank;
            term = (double)(i + 1) / (double)rank;
        }
        const int n = R - c0 < 64 ? (int)(R - c0) : 64;
        for (int l = 0; l < n; ++l) sum += __shfl(term, l, 64);
        if (c0 == 0) fr = __shfl(rank, 0, 64);
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) {
        ap[q] = R > 0 ? sum / (double)R : 0.0;
        first[q] = fr;
    }
}

int ranks_check(const void* queries, i64 Q, const void* gallery, i64 G, int dim, const int64_t* query_labels,
                const int64_t* gallery_labels, const int64_t* exclude, i64 idx_offset, const int64_t* offsets,
                const int64_t* offsets_host, const void* pos_keys, i64 nnz, const void* before, i64 query_block, const char* who,
                RanksArgs* a) {
    MI355_REQUIRE(queries && gallery, "%s: null queries/gallery pointer", who);
    MI355_REQUIRE(query_labels && gallery_labels, "%s: null query_labels/gallery_labels", who);
    MI355_REQUIRE(offsets, "%s: null offsets", who);
    MI355_REQUIRE(Q >= 1 && G >= 1 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    MI355_REQUIRE(Q <= INT_MAX && G < ((int64_t)1 << 31) - RK_BN, "%s: shape too large Q=%lld G=%lld", who, (long long)Q,
                  (long long)G);
    MI355_REQUIRE(nnz >= 0 && nnz <= Q * G, "%s: nnz=%lld outside [0, Q * G]", who, (long long)nnz);
    MI355_REQUIRE(nnz == 0 || (pos_keys && before), "%s: null pos_keys/before with nnz=%lld", who, (long long)nnz);
    MI355_REQUIRE(((uintptr_t)pos_keys & 7) == 0, "%s: pos_keys must be 8-byte aligned", who);
    MI355_REQUIRE(query_block >= 0, "%s: query_block=%lld < 0", who, (long long)query_block);
    if (offsets_host) {
        MI355_REQUIRE(offsets_host[0] == 0, "%s: offsets[0] = %lld, not 0", who, (long long)offsets_host[0]);
        for (i64 q = 0; q < Q; ++q) {
            const i64 n = offsets_host[q + 1] - offsets_host[q];
            MI355_REQUIRE(n >= 0 && n <= G, "%s: offsets must be monotone with at most G per query: query %lld has %lld", who,
                          (long long)q, (long long)n);
        }
        MI355_REQUIRE(offsets_host[Q] == nnz, "%s: offsets[Q] = %lld but nnz = %lld", who, (long long)offsets_host[Q], (long long)nnz);
    }
    a->qlab = (const i64*)query_labels;
    a->glab = (const i64*)gallery_labels;
    a->excl = (const i64*)exclude;
    a->idx_offset = idx_offset;
    a->offsets = (const i64*)offsets;
    a->keys = (const unsigned long long*)pos_keys;
    a->before = (unsigned*)before;
    return OK;
}

RanksArgs ranks_from(const RanksArgs& a, i64 q0) {
    RanksArgs r = a;
    r.qlab += q0;
    if (r.excl) r.excl += q0;
    r.offsets += q0;
    return r;
}

i64 ranks_query_block(i64 Q, i64 G, i64 query_block) {
    const i64 qb = roc_query_block(Q, G);
    return query_block > 0 && query_block < qb ? query_block : qb;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_rank_positives_keys(const int64_t* indices, const float* scores, int64_t nnz, int64_t idx_offset, uint64_t* keys,
                              void* stream) {
    MI355_REQUIRE(nnz >= 0, "rank_positives_keys: nnz=%lld < 0", (long long)nnz);
    MI355_REQUIRE(nnz == 0 || (indices && scores && keys), "rank_positives_keys: null pointer");
    if (nnz == 0) return OK;
    const unsigned blocks = (unsigned)(cdiv(nnz, 256) < 8192 ? cdiv(nnz, 256) : 8192);
    hipLaunchKernelGGL(k_ranks_keys, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const i64*)indices, scores, (i64)nnz,
                       (i64)idx_offset, (unsigned long long*)keys);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_rank_positives_finalize(const int64_t* offsets, const uint32_t* before, int64_t Q, int64_t nnz, int64_t* ranks, double* ap,
                                  int64_t* first_rank, void* stream) {
    const char* who = "rank_positives_finalize";
    MI355_REQUIRE(Q >= 1 && Q <= INT_MAX, "%s: Q=%lld outside [1, 2^31)", who, (long long)Q);
    MI355_REQUIRE(nnz >= 0, "%s: nnz=%lld < 0", who, (long long)nnz);
    MI355_REQUIRE(offsets && ap && first_rank, "%s: null offsets/ap/first_rank", who);
    MI355_REQUIRE(nnz == 0 || (before && ranks), "%s: null before/ranks with nnz=%lld", who, (long long)nnz);
    RoctxRange range("ranks/finalize");
    hipLaunchKernelGGL(k_ranks_finalize, dim3((unsigned)cdiv(Q, 4)), dim3(256), 0, (hipStream_t)stream, (const i64*)offsets, before,
                       (i64)Q, (i64*)ranks, ap, (i64*)first_rank);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
