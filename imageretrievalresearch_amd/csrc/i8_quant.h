// The int8 row quantiser and the split of a query into its two int8 planes (include/mi355_retrieval.h, the int8 block): what
// the exhaustive search (rank_i8.hip) and the scan of probed lists (ivf.hip) share, so that both make the same codes of a
// query and give a (query, row) pair the same bits.  gfx950 only.
#pragma once
#include "rank_common.h"

#include <float.h>

namespace mi355 {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int I8_KSTEP = 128;                 // k-step of the GEMM: one 128-byte segment of a stored row
constexpr int I8_MAX_DIM = 65536;             // 65536 * 127 * 127 < 2^31: the int32 sums are exact
static inline int i8_ld(int dim) { return (dim + I8_KSTEP - 1) / I8_KSTEP * I8_KSTEP; }

// ---- the row quantiser: scale and inverse scale of a row from its amax, then the code of one element
struct I8Quant {
    float scale, inv;
    bool zero;                                // every code is 0 (NaN row, zero row)
};
__device__ __forceinline__ I8Quant i8_quant(float amax, bool has_nan) {
    if (has_nan || !(amax <= FLT_MAX)) return {__uint_as_float(0x7fc00000u), 0.f, true};
    if (amax < 1e-30f) return {0.f, 0.f, true};
    return {amax / 127.0f, 127.0f / amax, false};
}
// clamp(rintf(x * m), -127, 127); the empty asm pins the fp32 product in a register, as scaled_f16 does
__device__ __forceinline__ int i8_code(float x, float m) {
    float p = x * m;
    asm volatile("" : "+v"(p));
    return (int)fminf(fmaxf(rintf(p), -127.0f), 127.0f);
}
// the fp32 row value x * r (the bits of l2_normalize_rows), pinned so that no later product is folded into it
__device__ __forceinline__ float i8_norm_elem(float x, float r) {
    float p = x * r;
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ unsigned pack4_i8(int a, int b, int c, int d) {
    return (unsigned)(a & 0xff) | ((unsigned)(b & 0xff) << 8) | ((unsigned)(c & 0xff) << 16) | ((unsigned)(d & 0xff) << 24);
}

// ---- the two planes of one element n of a normalised query with quantiser q (not q.zero): h = the row quantiser's code,
// l = the code of what it leaves, r = fmaf(-h, s_q, n), at 128 / s_q (lo_mul)
__device__ __forceinline__ void i8_split_elem(float n, const I8Quant& q, float lo_mul, int& h, int& l) {
    h = i8_code(n, q.inv);
    l = i8_code(__builtin_fmaf(-(float)h, q.scale, n), lo_mul);
}
__device__ __forceinline__ float i8_lo_mul(const I8Quant& q) { return q.zero ? 0.f : 128.0f / q.scale; }

// The float tail of every int8 score: the exact sums of the two planes, s_q and s_g
__device__ __forceinline__ float i8_score(int acc_hi, int acc_lo, float s_q, float s_g) {
    return (__builtin_fmaf((float)acc_lo, 0x1p-7f, (float)acc_hi) * s_q) * s_g;
}

}  // namespace mi355
