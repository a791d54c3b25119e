// Cosine range search (mi355_cosine_range*): the host side shared by the fp32 and fp16 entries (workspace, checks) and the
// compaction that turns the range pass's hits (rank_common.h: the RangeArgs epilogue; driver cosine_range in
// rank.hip) into a CSR result whose order does not depend on the order of the GEMM's atomics.  gfx950 only.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <limits.h>
#include <math.h>

namespace mi355 {

// hits of each query of the block: the sum of its ntx tile counts (one wave per query)
__global__ __launch_bounds__(256) void k_range_rows(const int* __restrict__ tcount, i64 qn, int ntx, i64* __restrict__ rowcnt) {
    const int lane = threadIdx.x & 63;
    const i64 q = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= qn) return;
    const int* c = tcount + q * ntx;
    i64 s = 0;
    for (int t = lane; t < ntx; t += 64) s += c[t];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) rowcnt[q] = s;
}

// out[q] = off + rowcnt[0] + .. + rowcnt[q] (inclusive), q < n: one workgroup, each thread a contiguous run
__global__ __launch_bounds__(1024) void k_range_scan(const i64* __restrict__ rowcnt, i64 n, i64 off, i64* __restrict__ out) {
    __shared__ i64 part[1024];
    const int tid = threadIdx.x;
    const i64 per = (n + 1023) / 1024, b0 = tid * per < n ? tid * per : n, b1 = b0 + per < n ? b0 + per : n;
    i64 s = 0;
    for (i64 i = b0; i < b1; ++i) s += rowcnt[i];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {              // Hillis-Steele over the 1024 run sums
        const i64 v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    s = off + part[tid] - s;                           // exclusive prefix of this run
    for (i64 i = b0; i < b1; ++i) {
        s += rowcnt[i];
        out[i] = s;
    }
}

// Every (query, tile) chunk of raw to canon in tile order, from the query's CSR offset: one wave per query, a lane per tile
// (an exclusive scan of 64 tile counts at a time), each lane copies its chunk (at most 128 entries, in column order)
__global__ __launch_bounds__(256) void k_range_gather(const i64* __restrict__ tstart, const int* __restrict__ tcount, i64 qn, int ntx,
                                                      const i64* __restrict__ offsets, const unsigned long long* __restrict__ raw,
                                                      unsigned long long* __restrict__ canon) {
    const int lane = threadIdx.x & 63;
    const i64 q = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= qn) return;
    i64 dst = offsets[q];
    for (int t0 = 0; t0 < ntx; t0 += 64) {
        const int t = t0 + lane;
        const int c = t < ntx ? tcount[q * ntx + t] : 0;
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (c > 0) {
            const unsigned long long* src = raw + tstart[q * ntx + t];
            unsigned long long* o = canon + dst + (incl - c);
            for (int e = 0; e < c; ++e) o[e] = src[e];
        }
        dst += __shfl(incl, 63, 64);
    }
}

// canon -> indices (local column + idx_offset) and scores (the fp32 bits as the epilogue computed them)
__global__ __launch_bounds__(256) void k_range_emit(const unsigned long long* __restrict__ canon, i64 nnz, i64 idx_offset,
                                                    i64* __restrict__ indices, float* __restrict__ scores) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nnz; i += stride) {
        const unsigned long long e = canon[i];
        indices[i] = (i64)(unsigned)(e & 0xffffffffull) + idx_offset;
        scores[i] = __uint_as_float((unsigned)(e >> 32));
    }
}

i64 range_query_block(i64 Q, i64 G) {
    // the split planes of one call stay those of mi355_cosine_scores (256 * 64 queries), the table [qb][ntx] about 2^23
    // entries (12 B each), and the 1-D grid < 2^31
    const i64 ntx = cdiv(G, RK_BN) > 0 ? cdiv(G, RK_BN) : 1;
    i64 qb = ((i64)1 << 23) / ntx / 128 * 128;
    if (qb < 128) qb = 128;
    if (qb > 256 * 64) qb = 256 * 64;
    while (qb > 128 && ntx * cdiv(qb, 64) >= INT_MAX) qb /= 2;
    return qb < Q ? qb : Q;
}

RangeWs range_carve(void* ws, i64 Q, i64 G, int D, size_t (*planes_bytes)(i64, int), bool need_ginv) {
    RangeWs r{};
    WsCarver c(ws);
    r.offsets = (i64*)c.take((size_t)(Q + 1) * sizeof(i64));
    if (Q > 0 && G > 0) {
        r.cursor = (unsigned long long*)c.take(sizeof(unsigned long long));
        r.w = carve(c.next(), Q, G, D, 0, planes_bytes, need_ginv, false);
        c.take(r.w.total - 256);                       // (carve's base is already 256-aligned here: its slack is not needed)
        const i64 qb = range_query_block(Q, G);
        const size_t cells = (size_t)qb * cdiv(G, RK_BN);
        r.tstart = (i64*)c.take(cells * sizeof(i64));
        r.tcount = (int*)c.take(cells * sizeof(int));
        r.rowcnt = (i64*)c.take((size_t)qb * sizeof(i64));
    }
    r.total = c.total();
    return r;
}

int range_check(const void* queries, i64 Q, const void* gallery, i64 G, int dim, double threshold,
                const mi355_rank_filter* filter, i64 idx_offset, void* candidates, i64 capacity, const int64_t* nnz,
                const char* who, RankFilter* f) {
    MI355_REQUIRE(queries && gallery, "%s: null queries/gallery pointer", who);
    MI355_REQUIRE(nnz, "%s: null nnz (host pointer)", who);
    MI355_REQUIRE(Q >= 0 && G >= 0 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    MI355_REQUIRE(Q <= INT_MAX && G < ((int64_t)1 << 31) - RK_BN, "%s: shape too large Q=%lld G=%lld", who, (long long)Q,
                  (long long)G);
    MI355_REQUIRE(isfinite(threshold), "%s: threshold is not finite (%g)", who, threshold);
    MI355_REQUIRE(capacity >= 0, "%s: capacity=%lld < 0", who, (long long)capacity);
    MI355_REQUIRE(candidates || capacity == 0, "%s: null candidates with capacity %lld", who, (long long)capacity);
    MI355_REQUIRE(((uintptr_t)candidates & 7) == 0, "%s: candidates must be 8-byte aligned", who);
    *f = RankFilter{};
    f->idx_offset = idx_offset;
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, f)) return e;
    return OK;
}

int range_empty(const RangeWs& w, i64 Q, int64_t* nnz, hipStream_t st) {
    MI355_CHECK_HIP(hipMemsetAsync(w.offsets, 0, (size_t)(Q + 1) * sizeof(i64), st));
    *nnz = 0;
    return OK;
}

int range_compact_block(const RangeWs& w, i64 q0, i64 qn, i64 G, i64 off, const unsigned long long* raw,
                        unsigned long long* canon, hipStream_t st) {
    const int ntx = cdiv(G, RK_BN);
    hipLaunchKernelGGL(k_range_rows, dim3((unsigned)cdiv(qn, 4)), dim3(256), 0, st, (const int*)w.tcount, qn, ntx, w.rowcnt);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(1024), 0, st, (const i64*)w.rowcnt, qn, off, w.offsets + q0 + 1);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_range_gather, dim3((unsigned)cdiv(qn, 4)), dim3(256), 0, st, (const i64*)w.tstart, (const int*)w.tcount, qn,
                       ntx, (const i64*)(w.offsets + q0), raw, canon);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_range_compact(const void* candidates, int64_t capacity, int64_t Q, int64_t nnz, int64_t idx_offset, const void* workspace,
                        size_t workspace_bytes, int64_t* offsets, int64_t* indices, float* scores, void* stream) {
    const char* who = "range_compact";
    MI355_REQUIRE(Q >= 0, "%s: Q=%lld < 0", who, (long long)Q);
    MI355_REQUIRE(nnz >= 0 && nnz <= capacity, "%s: nnz=%lld outside [0, capacity=%lld]: search again with capacity >= nnz", who,
                  (long long)nnz, (long long)capacity);
    MI355_REQUIRE(candidates || nnz == 0, "%s: null candidates", who);
    MI355_REQUIRE(offsets, "%s: null offsets", who);
    MI355_REQUIRE((indices && scores) || nnz == 0, "%s: null indices/scores", who);
    const size_t need = align_up((size_t)(Q + 1) * sizeof(i64), 256) + 256;
    MI355_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const RangeWs w = range_carve(const_cast<void*>(workspace), Q, 0, 1, nullptr, false);   // (the offsets lead every layout)
    MI355_CHECK_HIP(hipMemcpyAsync(offsets, w.offsets, (size_t)(Q + 1) * sizeof(i64), hipMemcpyDeviceToDevice, st));
    if (nnz == 0) return OK;
    const unsigned long long* canon = (const unsigned long long*)candidates + capacity;
    const unsigned blocks = (unsigned)(cdiv(nnz, 256) < 8192 ? cdiv(nnz, 256) : 8192);
    hipLaunchKernelGGL(k_range_emit, dim3(blocks), dim3(256), 0, st, canon, (i64)nnz, (i64)idx_offset, (i64*)indices, scores);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
