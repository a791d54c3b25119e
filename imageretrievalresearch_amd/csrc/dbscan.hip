// DBSCAN and threshold components beside the two sweeps of the cosine GEMM (rank_common.h: DegreeEpi, LinkEpi and the
// union-find; driver dbscan_sweep in rank.hip): the state a clustering keeps between its calls (mi355_dbscan_init), the checks
// of the sweeps, and the finishing kernel that turns parent[] / border[] into one root per row (mi355_dbscan_finish).  Every
// result is the same bits on every run: the degrees are integer sums, a component's root is its smallest core row and a
// border row's choice is the maximum of a key.  gfx950 only.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <limits.h>
#include <math.h>

namespace mi355 {

__global__ __launch_bounds__(256) void k_dbscan_iota(int* __restrict__ parent, i64 N) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) parent[i] = (int)i;
}

// The root above x.  A launch of its own: the link sweeps ended before it and nothing writes parent[] here, so plain loads.
__device__ __forceinline__ int dbscan_root(const int* __restrict__ parent, int x) {
    int p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

// root[i] = the root (smallest core row) of the cluster of row i: a core row's own component; a non-core row's chosen core
// row's (the low word of its border key, complemented); -1 for a non-core row that no core row offered itself to (noise).
__global__ __launch_bounds__(256) void k_dbscan_finish(const int* __restrict__ degree, const int* __restrict__ parent,
                                                       const unsigned long long* __restrict__ border, i64 N, int min_samples,
                                                       i64* __restrict__ root, unsigned char* __restrict__ core) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
        const bool c = degree[i] >= min_samples;
        const unsigned long long b = border[i];
        core[i] = c ? 1 : 0;
        if (c) root[i] = dbscan_root(parent, (int)i);
        else {
            const unsigned chosen = ~(unsigned)(b & 0xffffffffull);
            root[i] = b && chosen < N ? (i64)dbscan_root(parent, (int)chosen) : -1;
        }
    }
}

int dbscan_check(const void* queries, i64 q0, i64 rows, const void* gallery, i64 N, int dim, double threshold, int min_samples,
                 const void* degree, const void* parent, const void* border, bool link, const char* who) {
    MI355_REQUIRE(queries && gallery, "%s: null queries/gallery pointer", who);
    MI355_REQUIRE(degree, "%s: null degree", who);
    MI355_REQUIRE(!link || (parent && border), "%s: null parent/border", who);
    MI355_REQUIRE(N >= 1 && dim >= 1, "%s: bad shape N=%lld dim=%d", who, (long long)N, dim);
    MI355_REQUIRE(N < ((int64_t)1 << 31) - RK_BN, "%s: shape too large N=%lld", who, (long long)N);
    MI355_REQUIRE(q0 >= 0 && rows >= 0 && q0 <= N && rows <= N - q0, "%s: rows [%lld, %lld + %lld) outside the N=%lld rows", who,
                  (long long)q0, (long long)q0, (long long)rows, (long long)N);
    MI355_REQUIRE(isfinite(threshold), "%s: threshold is not finite (%g)", who, threshold);
    MI355_REQUIRE(min_samples >= 1, "%s: min_samples=%d must be >= 1", who, min_samples);
    MI355_REQUIRE(((uintptr_t)border & 7) == 0 && (((uintptr_t)degree | (uintptr_t)parent) & 3) == 0,
                  "%s: degree/parent must be 4-byte and border 8-byte aligned", who);
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_dbscan_init(int64_t N, int32_t* degree, int32_t* parent, uint64_t* border, void* stream) {
    const char* who = "dbscan_init";
    MI355_REQUIRE(N >= 1 && N < ((int64_t)1 << 31) - RK_BN, "%s: N=%lld outside [1, 2^31 - 128)", who, (long long)N);
    MI355_REQUIRE(degree && parent && border, "%s: null degree/parent/border", who);
    MI355_REQUIRE(((uintptr_t)border & 7) == 0 && (((uintptr_t)degree | (uintptr_t)parent) & 3) == 0,
                  "%s: degree/parent must be 4-byte and border 8-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    MI355_CHECK_HIP(hipMemsetAsync(degree, 0, (size_t)N * sizeof(int32_t), st));
    MI355_CHECK_HIP(hipMemsetAsync(border, 0, (size_t)N * sizeof(uint64_t), st));
    const unsigned blocks = (unsigned)(cdiv(N, 256) < 8192 ? cdiv(N, 256) : 8192);
    hipLaunchKernelGGL(k_dbscan_iota, dim3(blocks), dim3(256), 0, st, (int*)parent, (i64)N);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_dbscan_finish(int64_t N, int min_samples, const int32_t* degree, const int32_t* parent, const uint64_t* border,
                        int64_t* root, uint8_t* core, void* stream) {
    const char* who = "dbscan_finish";
    MI355_REQUIRE(N >= 1 && N < ((int64_t)1 << 31) - RK_BN, "%s: N=%lld outside [1, 2^31 - 128)", who, (long long)N);
    MI355_REQUIRE(min_samples >= 1, "%s: min_samples=%d must be >= 1", who, min_samples);
    MI355_REQUIRE(degree && parent && border, "%s: null degree/parent/border", who);
    MI355_REQUIRE(root && core, "%s: null root/core output", who);
    MI355_REQUIRE(((uintptr_t)border & 7) == 0 && (((uintptr_t)degree | (uintptr_t)parent) & 3) == 0 && ((uintptr_t)root & 7) == 0,
                  "%s: degree/parent must be 4-byte, border/root 8-byte aligned", who);
    RoctxRange range("dbscan/finish");
    const unsigned blocks = (unsigned)(cdiv(N, 256) < 8192 ? cdiv(N, 256) : 8192);
    hipLaunchKernelGGL(k_dbscan_finish, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const int*)degree, (const int*)parent,
                       (const unsigned long long*)border, (i64)N, min_samples, (i64*)root, (unsigned char*)core);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
