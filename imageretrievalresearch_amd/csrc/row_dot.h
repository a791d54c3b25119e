// The fp32 dot of one resident row with up to NQ queries, one wave per row: shared by the IVF scan (ivf.hip) and the candidate
// rescoring (pq.hip), so that both give a (query, row) pair the same bits.  Lane i takes the elements [4u, 4u + 4) (fp16 rows:
// [8u, 8u + 8), widened exactly) of the units u = i, i + 64, ... in ascending order, one fused multiply-add each; the caller
// reduces the 64 partial sums with wave_sum.  The order depends on dim alone.  gfx950 only.
#pragma once
#include "rank_common.h"

namespace mi355 {

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// One unit of a row per lane and load: 4 floats, or 8 halves widened exactly.  The elements past dim read as zero (an fp16
// row's padding is zero as stored).
template <bool VEC>
__device__ __forceinline__ f32x4 load_unit(const float* __restrict__ row, int u, int dim) {
    if constexpr (VEC) return reinterpret_cast<const f32x4*>(row)[u];
    f32x4 v;
    const int e = u * 4;
    v.x = row[e];                                   // u < cdiv(dim, 4): the first element exists
    v.y = e + 1 < dim ? row[e + 1] : 0.f;
    v.z = e + 2 < dim ? row[e + 2] : 0.f;
    v.w = e + 3 < dim ? row[e + 3] : 0.f;
    return v;
}
// acc + v . u, element by element in ascending order: one fused multiply-add each, so the bits do not depend on how the
// compiler contracts the surrounding code
__device__ __forceinline__ float dot_unit(float acc, const f32x4 v, const float* __restrict__ u) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(u);
    acc = __builtin_fmaf(v.x, w.x, acc);
    acc = __builtin_fmaf(v.y, w.y, acc);
    acc = __builtin_fmaf(v.z, w.z, acc);
    acc = __builtin_fmaf(v.w, w.w, acc);
    return acc;
}

// acc[q] += row g . query q of the group (qs [NQ][ldq] in LDS, zero from dim on) over this lane's units, up to four loads in
// flight.  a: anything with rows (the rows' base), ld (elements between rows), ldq (dim rounded up to a unit) and dim.
template <int NQ, bool F16, bool VEC, class Args>
__device__ __forceinline__ void row_dot(const Args& a, i64 g, const float* __restrict__ qs, int lane, float (&acc)[NQ]) {
    constexpr int UNIT = F16 ? 8 : 4;
    const int nunits = a.ldq / UNIT, ldq = a.ldq;
    if constexpr (F16) {
        const f16x8* row = reinterpret_cast<const f16x8*>((const f16*)a.rows + g * a.ld);
        for (int c0 = 0; c0 < nunits; c0 += 4 * 64) {
            f16x8 h[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                h[u] = c < nunits ? row[c] : (f16x8){};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                if (c < nunits) {
                    const f32x4 lo = {(float)h[u][0], (float)h[u][1], (float)h[u][2], (float)h[u][3]};
                    const f32x4 hi = {(float)h[u][4], (float)h[u][5], (float)h[u][6], (float)h[u][7]};
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        acc[q] = dot_unit(acc[q], lo, &qs[q * ldq + c * 8]);
                        acc[q] = dot_unit(acc[q], hi, &qs[q * ldq + c * 8 + 4]);
                    }
                }
            }
        }
    } else {
        const float* row = (const float*)a.rows + g * a.ld;
        for (int c0 = 0; c0 < nunits; c0 += 4 * 64) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                v[u] = c < nunits ? load_unit<VEC>(row, c, a.dim) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                if (c < nunits) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] = dot_unit(acc[q], v[u], &qs[q * ldq + c * 4]);
                }
            }
        }
    }
}

// Floats of one query in LDS: dim rounded up to a unit
static inline int row_dot_ldq(int dim, bool f16rows) { const int u = f16rows ? 8 : 4; return (dim + u - 1) / u * u; }

}  // namespace mi355
