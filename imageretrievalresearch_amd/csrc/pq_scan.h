// What the scans over product-quantised rows share (pq.hip: every row of the gallery; ivfpq.hip: the rows of the probed lists):
// the shape rules, the threads of a scan workgroup, the table in LDS and the lookups of one row.  The arithmetic is specified
// bit for bit in include/mi355_retrieval.h.  gfx950 only.
#pragma once
#include "rank_common.h"

namespace mi355 {

constexpr int PQ_CENTROIDS = 256;
constexpr int PQ_MAX_M = 128;
constexpr int PQ_MAX_DSUB = 64;
// Threads of a scan workgroup (a template argument NT): the LDS a table takes bounds the workgroups per CU, so a larger table is
// shared by more waves - 16 to 24 waves per CU in every case (measured, DESIGN.md section 5: at M = 96 1024 threads are 1.4x
// faster than 256, at M = 48 they are 1.2x slower than 256)
static int pq_threads(int M) { return M <= 40 ? 256 : M <= 80 ? 512 : 1024; }
constexpr i64 PQ_QBLOCK = 256;              // queries of one table / scan launch (the tables of a block: 256 * M KB)
constexpr i64 PQ_SLAB_FLOATS = (i64)1 << 27;   // the score slab of one query block stays under 512 MB

// ---- the lookups of one row: tab [M][256] in LDS, the row's M codes read 16 bytes at a time (VEC: M % 16 == 0, so every row
// of a 16-byte aligned base is aligned) or 4 (M % 4 == 0).  Byte m of a unit goes to accumulator m % 4 (a unit starts at a
// multiple of 4).
__device__ __forceinline__ void pq_lookup4(const float* t, unsigned w, float& a0, float& a1, float& a2, float& a3) {
    a0 = __fadd_rn(a0, t[w & 255u]);
    a1 = __fadd_rn(a1, t[PQ_CENTROIDS + ((w >> 8) & 255u)]);
    a2 = __fadd_rn(a2, t[2 * PQ_CENTROIDS + ((w >> 16) & 255u)]);
    a3 = __fadd_rn(a3, t[3 * PQ_CENTROIDS + (w >> 24)]);
}
template <bool VEC>
__device__ __forceinline__ float pq_score(const float* tab, const unsigned char* __restrict__ codes, i64 g, int M) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if constexpr (VEC) {
        const uint4* row = reinterpret_cast<const uint4*>(codes + g * M);
        for (int u = 0; u < M / 16; ++u) {
            const uint4 w = row[u];
            const float* t = tab + u * 16 * PQ_CENTROIDS;
            pq_lookup4(t, w.x, a0, a1, a2, a3);
            pq_lookup4(t + 4 * PQ_CENTROIDS, w.y, a0, a1, a2, a3);
            pq_lookup4(t + 8 * PQ_CENTROIDS, w.z, a0, a1, a2, a3);
            pq_lookup4(t + 12 * PQ_CENTROIDS, w.w, a0, a1, a2, a3);
        }
    } else {
        const unsigned* row = reinterpret_cast<const unsigned*>(codes + g * M);
        for (int u = 0; u < M / 4; ++u) pq_lookup4(tab + u * 4 * PQ_CENTROIDS, row[u], a0, a1, a2, a3);
    }
    return __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
}
// The table of query blockIdx.y of T into tab; ends in a barrier
template <int NT>
__device__ __forceinline__ void pq_load_table(float* tab, const float* __restrict__ T, int M) {
    const f32x4* src = reinterpret_cast<const f32x4*>(T + (size_t)blockIdx.y * M * PQ_CENTROIDS);
    for (int i = threadIdx.x; i < M * (PQ_CENTROIDS / 4); i += NT) reinterpret_cast<f32x4*>(tab)[i] = src[i];
    __syncthreads();
}

// ---- host side
static bool pq_shape_ok(int dim, int M) {
    return M >= 4 && M <= PQ_MAX_M && M % 4 == 0 && dim >= 1 && dim % M == 0 && dim / M <= PQ_MAX_DSUB;
}
static int pq_check_shape(const char* who, int dim, int M) {
    MI355_REQUIRE(M >= 4 && M <= PQ_MAX_M && M % 4 == 0, "%s: M=%d must be a multiple of 4 in [4, %d]", who, M, PQ_MAX_M);
    MI355_REQUIRE(dim >= 1 && dim % M == 0, "%s: dim=%d must be a positive multiple of M=%d", who, dim, M);
    MI355_REQUIRE(dim / M <= PQ_MAX_DSUB, "%s: dsub = dim / M = %d exceeds %d", who, dim / M, PQ_MAX_DSUB);
    return OK;
}
// k_pq_table (pq.hip): T [qn][M][256] of the normalised queries qn_rows [qn][dim]
int launch_table(const float* qn_rows, i64 qn, int dim, const float* cb, int M, float* T, hipStream_t st);

}  // namespace mi355
