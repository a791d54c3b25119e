// 4-bit resident gallery: e2m1 rows, two codes per byte, with one fp32 multiplier per row, and the cosine / top-k / range search
// over them on v_mfma_scale_f32_32x32x64_f8f6f4 with both operands fp4.  gfx950 only.
//
// Numerical contract (include/mi355_retrieval.h, the fp4 block).  "fp32" = one IEEE rounding per named operation.
//   * e2m1(a): |a| to the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, a tie to the even index; sign in bit 3, no negative zero.
//   * row quantiser: n = the fp32 row mi355_l2_normalize_rows writes for x, amax = max |n_i|.  A NaN element or a non-finite
//     amax: mult = NaN, codes 0.  amax < 1e-30: mult = 0, codes 0.  Else inv = 6 / amax, code_i = e2m1(n_i * inv), n2 = sum of
//     (2 value(code_i))^2 (an integer), mult = 1 / sqrt(0.25 * n2) = 1 / |value(codes)|.  Dimension 2j is the low nibble of byte
//     j; ld = ceil(dim / 2) rounded up to a multiple of 128 bytes, nibbles from dim on are 0.
//   * query planes, per call, from qn = l2_normalize_rows(q): s_q = amax_q / 6, hi_i = e2m1(qn_i * (6 / amax_q)),
//     r_i = fmaf(-value(hi_i), s_q, qn_i) / s_q, lo_i = e2m1(4 * r_i) (|value(lo_i)| <= 4).
//   * score: acc_hi = sum value(hi_i) value(c_i), acc_lo = sum value(lo_i) value(c_i): every product is a multiple of 0.25 of
//     magnitude <= 36, so every partial sum is exact in fp32 in any order (dim <= 65536); t = fmaf(acc_lo, 0.25, acc_hi);
//     score = (t * s_q) * mult.  A NaN row scores NaN, a zero row 0, a NaN query NaN everywhere.
//   * the sums do not depend on any summation order, so the GEMV (Q <= 4), both tile sizes of the GEMM, its two launches and
//     every epilogue return the SAME bits for a (query, row) pair.
//   * order, ties, NaN, pads: the selection of mi355_rank_topk (rank_common.h).
#include "i8_quant.h"
#include "rows_gemm.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int FP4_MAX_DIM = 65536;            // 36 * 65536 * 4 < 2^24: the fp32 sums of multiples of 0.25 are exact
static inline int fp4_ld(int dim) { return ((dim + 1) / 2 + ROWS_KSTEP - 1) / ROWS_KSTEP * ROWS_KSTEP; }

// ---- e2m1: the magnitude index of |a| (nearest, a tie to the even index), the code of a, and a code's value
__device__ __forceinline__ int e2m1_index(float m) {
    return (m > 0.25f) + (m >= 0.75f) + (m > 1.25f) + (m >= 1.75f) + (m > 2.5f) + (m >= 3.5f) + (m > 5.0f);
}
__device__ __forceinline__ unsigned e2m1(float a) {
    const int m = e2m1_index(fabsf(a));
    return (unsigned)m | ((a < 0.f && m) ? 8u : 0u);
}
__device__ __forceinline__ float e2m1_value(unsigned code) {
    const int m = code & 7;
    const float v = m < 5 ? 0.5f * (float)m : m == 5 ? 3.0f : m == 6 ? 4.0f : 6.0f;
    return code & 8 ? -v : v;
}
// 2 * value(code) as an integer: {0, 1, 2, 3, 4, 6, 8, 12}, signed
__device__ __forceinline__ int e2m1_twice(unsigned code) {
    const int m = code & 7;
    const int v = m < 5 ? m : m == 5 ? 6 : m == 6 ? 8 : 12;
    return code & 8 ? -v : v;
}
// x * m in fp32, pinned in a register so that no later operation is fused into it
__device__ __forceinline__ float fp4_scaled(float x, float m) {
    float p = x * m;
    asm volatile("" : "+v"(p));
    return p;
}

// ---- the quantiser of a row (or of a query) from its amax
struct Fp4Quant {
    float scale, inv;                         // amax / 6 and 6 / amax (rows use inv only); scale = NaN / 0 for a NaN / zero row
    bool zero;                                // every code is 0 (NaN row, zero row)
};
__device__ __forceinline__ Fp4Quant fp4_quant(float amax, bool has_nan) {
    if (has_nan || !(amax <= FLT_MAX)) return {__uint_as_float(0x7fc00000u), 0.f, true};
    if (amax < 1e-30f) return {0.f, 0.f, true};
    return {amax / 6.0f, 6.0f / amax, false};
}

// amax and the NaN flag of the row x * r over the wave
__device__ __forceinline__ Fp4Quant fp4_row_quant(const float* __restrict__ x, int dim, float r, int vec, int lane) {
    float amax = 0.f;
    bool nan = false;
    if (vec) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        for (int i = lane; i < dim / 4; i += 64) {
            const f32x4 v = x4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float n = i8_norm_elem(v[e], r);
                nan = nan || n != n;
                amax = fmaxf(amax, fabsf(n));
            }
        }
    } else {
        for (int i = lane; i < dim; i += 64) {
            const float n = i8_norm_elem(x[i], r);
            nan = nan || n != n;
            amax = fmaxf(amax, fabsf(n));
        }
    }
    return fp4_quant(wave_max(amax), __ballot(nan) != 0ull);
}

// the eight values x[k0 .. k0 + 7] * r of a row of dim elements, zeros from dim on (vec: dim % 4 == 0, x 16-byte aligned)
__device__ __forceinline__ void fp4_load8(const float* __restrict__ x, int k0, int dim, float r, int vec, float (&n)[8]) {
    if (vec) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k0 + 4 * h < dim) v = *reinterpret_cast<const f32x4*>(x + k0 + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) n[4 * h + e] = i8_norm_elem(v[e], r);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) n[e] = k0 + e < dim ? i8_norm_elem(x[k0 + e], r) : 0.f;
    }
}

// =====================================================================================
// fp32 rows -> packed e2m1 codes, padded to ld bytes with zeros, and one multiplier per row.  One wave per row: the norm with
// row_inv_norm, amax by wave reduction, then the codes (a lane packs eight dimensions into a word) and n2 by an integer wave
// reduction.  Appendable: converting n rows to codes + r * ld, mults + r writes rows r .. r+n-1.
// =====================================================================================
__global__ __launch_bounds__(256) void k_rows_to_fp4(const float* __restrict__ in, unsigned char* __restrict__ codes,
                                                     float* __restrict__ mults, i64 rows, int dim, int ld, float eps,
                                                     int normalize, int vec) {
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = in + row * dim;
    const float r = normalize ? row_inv_norm(x, dim, eps, vec, lane) : 1.0f;
    const Fp4Quant q = fp4_row_quant(x, dim, r, vec, lane);
    unsigned* y = reinterpret_cast<unsigned*>(codes + row * ld);
    int n2 = 0;
    for (int i = lane; i < ld / 4; i += 64) {              // word i: dimensions 8i .. 8i + 7
        unsigned w = 0u;
        if (8 * i < dim && !q.zero) {
            float n[8];
            fp4_load8(x, 8 * i, dim, r, vec, n);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned c = e2m1(fp4_scaled(n[e], q.inv));
                const int t = e2m1_twice(c);
                n2 += t * t;
                w |= c << (4 * e);
            }
        }
        y[i] = w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n2 += __shfl_xor(n2, o, 64);
    if (lane == 0) {
        float m = q.scale;                                 // NaN row: NaN, zero row: 0
        if (!q.zero) {
            // fp32 square root and division, correctly rounded: the double results rounded to fp32 are (53 >= 2 * 24 + 2)
            const float s = (float)sqrt((double)(0.25f * (float)n2));
            m = n2 ? (float)(1.0 / (double)s) : 0.f;
        }
        mults[row] = m;
    }
}

// =====================================================================================
// Normalised queries -> their two e2m1 planes in MFMA-fragment order and s_q per query:
// Qs[row block of 32][k sub-step of 64 dims][plane hi, lo][lane][16 B], lane = row + 32 * (k half): the lane's 16 bytes are the 32
// consecutive dimensions of its half of the sub-step.  A GEMM k-step of 128 bytes of a stored row (256 dimensions) is then 8 KB
// per row block, eight 1 KB pieces that LDS-DMA moves as they are.  One wave per row of the rows_pad (whole 128-row tiles) rows;
// rows >= Q and dimensions >= D are zero, sq 0.
// =====================================================================================
__global__ __launch_bounds__(256) void k_split_queries_fp4(const float* __restrict__ Qn, unsigned char* __restrict__ Qs,
                                                           float* __restrict__ sq, int Q, int D, int n_sub, int rows_pad, int vec) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_pad) return;
    const float* x = Qn + (i64)row * D;
    Fp4Quant q = {0.f, 0.f, true};
    if (row < Q) q = fp4_row_quant(x, D, 1.0f, vec, lane);
    if (lane == 0) sq[row] = q.scale;
    unsigned char* base = Qs + (size_t)(row >> 5) * n_sub * 2048 + (row & 31) * 16;
    for (int c = lane; c < 2 * n_sub; c += 64) {           // 16-byte chunk c: sub-step c / 2, k half c % 2, dimensions 32c ..
        unsigned hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
        if (!q.zero) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int k0 = c * 32 + w * 8;
                if (k0 >= D) break;
                float n[8];
                fp4_load8(x, k0, D, 1.0f, vec, n);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned h = e2m1(fp4_scaled(n[e], q.inv));
                    float res = __builtin_fmaf(-e2m1_value(h), q.scale, n[e]) / q.scale;
                    asm volatile("" : "+v"(res));
                    hi[w] |= h << (4 * e);
                    lo[w] |= e2m1(4.0f * res) << (4 * e);
                }
            }
        }
        unsigned char* o = base + (size_t)(c >> 1) * 2048 + (c & 1) * 512;
        *reinterpret_cast<i32x4*>(o) = (i32x4){(int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        *reinterpret_cast<i32x4*>(o + 1024) = (i32x4){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3]};
    }
}

// =====================================================================================
// cosine GEMM over fp4 rows: the DMA-ring loop of rows_gemm.h with 32 codes per fragment on v_mfma_scale_f32_32x32x64_f8f6f4 (a
// sub-step is 64 dimensions, 32 bytes of a stored row), both operands fp4 (cbsz = blgp = 4) and both block scales 2^0 (the E8M0
// byte 0x7f in every byte of the scale operand, so the byte select does not matter); fp32 accumulators that hold exact sums,
// and the tail t = fmaf(acc_lo, 0.25, acc_hi), then t * s_q per accumulator row; the epilogue's acc * ginv[col] is the
// multiply by mult.  (sq holds whole 128-row tiles: rows >= Q read 0.)
// Fragment map: a lane's A and B fragments of a sub-step are the SAME 32 consecutive dimensions (its half of the sub-step),
// nibble for nibble.  The MFMA pairs A and B nibbles by (lane half, nibble), and every partial sum is exactly representable,
// so whichever k the hardware calls them, and in whatever order it adds them, the result is the exact dot product.
// =====================================================================================
struct Fp4Tile {
    typedef i32x4 Frag;
    typedef f32x16 Acc;
    const float* __restrict__ sq;       // s_q of the call's queries
    const float* __restrict__ mults;    // mult of the gallery rows
    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
        const i32x8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
        return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    }
    __device__ __forceinline__ void tail(const Acc (&hi)[2], const Acc (&lo)[2], f32x16 (&acc)[2], int row0, int lane) const {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = sq[row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j][r] = __builtin_fmaf(lo[j][r], 0.25f, hi[j][r]) * s;
        }
    }
    __device__ __forceinline__ const float* ginv() const { return mults; }
};

template <int MT, int FK>
__global__ __launch_bounds__(256) void k_cos_gemm_fp4(const unsigned char* __restrict__ Qs, const float* __restrict__ sq,
                                                      const unsigned char* __restrict__ Gal, const float* __restrict__ mults, int Q,
                                                      i64 G, int ld, int x0, int ntx, int xtiles, int ny, PlainEpi<FK> epi) {
    rows_gemm_tile<Fp4Tile, MT>((const char*)Qs, (const char*)Gal, Fp4Tile{sq, mults}, Q, G, ld, x0, ntx, xtiles, ny, epi);
}
// Every other epilogue (filtered selection, range): the same loop
template <int MT, class Epi>
__global__ __launch_bounds__(256) void k_cos_gemm_fp4_epi(const unsigned char* __restrict__ Qs, const float* __restrict__ sq,
                                                          const unsigned char* __restrict__ Gal, const float* __restrict__ mults,
                                                          int Q, i64 G, int ld, int x0, int ntx, int xtiles, int ny, Epi epi) {
    rows_gemm_tile<Fp4Tile, MT>((const char*)Qs, (const char*)Gal, Fp4Tile{sq, mults}, Q, G, ld, x0, ntx, xtiles, ny, epi);
}

// =====================================================================================
// Few queries (Q <= 4): a GEMV bound by streaming the gallery once (ld bytes per row).  A wave takes GEMV_ROWS consecutive
// rows per pass, 16 bytes (32 codes) per lane per load and one load per row in flight per lane (a row of D = 1536 is 48 loads:
// one row at a time would leave a lane waiting on a single load), and reads a query's fragment from LDS once for those rows.
// Codes become int8 values 2 * value(code), {0, +-1, 2, 3, 4, 6, 8, 12}, by a 16-entry lookup: two v_perm_b32 over constant
// registers (the positive and the negative half of the table) and a bit select on the sign bits; a word of eight codes gives a
// word of its even and a word of its odd nibbles.
// A query sits in LDS as ONE int8 row [NQ][2 * ld], made once per block from the two planes the GEMM reads: 8 hi + 2 lo of the
// values (|.| <= 56), decoded in the same nibble order.  With P = sum (8 hi + 2 lo)(2 c), an exact integer below
// 56 * 12 * 65536 < 2^31, fmaf(acc_lo, 0.25, acc_hi) is the fp32 rounding of P / 16: float(P) * 2^-4 is the same bits as the
// GEMM's tail.  The integer sums are reduced over the wave in integers.
// =====================================================================================
template <unsigned LO, unsigned HI>     // the bytes of the table for magnitude indices 0..3 and 4..7
__device__ __forceinline__ unsigned fp4_lookup(unsigned sel) { return __builtin_amdgcn_perm(HI, LO, sel); }
// four nibbles, one per byte of x (each 0..15), to four int8: T times 2 * value; NEG = the bytes of the negated table
template <unsigned LO, unsigned HI, unsigned NLO, unsigned NHI>
__device__ __forceinline__ unsigned fp4_bytes(unsigned x) {
    const unsigned sel = x & 0x07070707u;
    const unsigned neg = ((x >> 3) & 0x01010101u) * 0xffu;             // 0xff in the bytes whose sign bit is set
    return (fp4_lookup<LO, HI>(sel) & ~neg) | (fp4_lookup<NLO, NHI>(sel) & neg);
}
// 2 * value: {0, 1, 2, 3 | 4, 6, 8, 12}
__device__ __forceinline__ unsigned fp4_twice4(unsigned x) { return fp4_bytes<0x03020100u, 0x0c080604u, 0xfdfeff00u, 0xf4f8fafcu>(x); }
// 8 * value: {0, 4, 8, 12 | 16, 24, 32, 48}
__device__ __forceinline__ unsigned fp4_eight4(unsigned x) { return fp4_bytes<0x0c080400u, 0x30201810u, 0xf4f8fc00u, 0xd0e0e8f0u>(x); }
// byte-wise a + b of int8 values whose sums stay within int8
__device__ __forceinline__ unsigned add4_i8(unsigned a, unsigned b) {
    return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
}

constexpr int GEMV_ROWS = 4;

template <int NQ>
__global__ __launch_bounds__(256) void k_cos_gemv_fp4(const unsigned char* __restrict__ Qs, const float* __restrict__ sq,
                                                      const unsigned char* __restrict__ Gal, const float* __restrict__ mults,
                                                      float* __restrict__ S, i64 G, int ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    i32x4* qs = reinterpret_cast<i32x4*>(smem);                  // [NQ][ld / 16 chunks][even words, odd words]
    const int nch = ld / 16;                                     // 16-byte chunks per stored row
    for (int i = threadIdx.x; i < NQ * nch; i += 256) {
        const int q = i / nch, c = i % nch;
        const unsigned char* src = Qs + ((size_t)((c >> 1) * 2) * 64 + (c & 1) * 32 + q) * 16;
        const i32x4 h = *reinterpret_cast<const i32x4*>(src), l = *reinterpret_cast<const i32x4*>(src + 1024);
        i32x4 ev, od;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned hw = (unsigned)h[e], lw = (unsigned)l[e];
            ev[e] = (int)add4_i8(fp4_eight4(hw & 0x0f0f0f0fu), fp4_twice4(lw & 0x0f0f0f0fu));
            od[e] = (int)add4_i8(fp4_eight4((hw >> 4) & 0x0f0f0f0fu), fp4_twice4((lw >> 4) & 0x0f0f0f0fu));
        }
        qs[2 * i] = ev;
        qs[2 * i + 1] = od;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const i64 wave_id = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const i64 nwaves = (i64)gridDim.x * 4;
    float s_q[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) s_q[q] = sq[q];
    for (i64 g0 = wave_id * GEMV_ROWS; g0 < G; g0 += nwaves * GEMV_ROWS) {
        const int nr = G - g0 < GEMV_ROWS ? (int)(G - g0) : GEMV_ROWS;
        const i32x4* row = reinterpret_cast<const i32x4*>(Gal + g0 * ld);
        int p[GEMV_ROWS][NQ];
#pragma unroll
        for (int r = 0; r < GEMV_ROWS; ++r)
#pragma unroll
            for (int q = 0; q < NQ; ++q) p[r][q] = 0;
        for (int c = lane; c < nch; c += 64) {
            i32x4 v[GEMV_ROWS];
#pragma unroll
            for (int r = 0; r < GEMV_ROWS; ++r) v[r] = r < nr ? row[(size_t)r * nch + c] : (i32x4){0, 0, 0, 0};
            i32x4 qe[NQ], qo[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                qe[q] = qs[2 * (q * nch + c)];
                qo[q] = qs[2 * (q * nch + c) + 1];
            }
#pragma unroll
            for (int r = 0; r < GEMV_ROWS; ++r) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned w = (unsigned)v[r][e];
                    const int ev = (int)fp4_twice4(w & 0x0f0f0f0fu), od = (int)fp4_twice4((w >> 4) & 0x0f0f0f0fu);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        p[r][q] = __builtin_amdgcn_sdot4(qe[q][e], ev, p[r][q], false);
                        p[r][q] = __builtin_amdgcn_sdot4(qo[q][e], od, p[r][q], false);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < GEMV_ROWS; ++r) {
            const float m = r < nr ? mults[g0 + r] : 0.f;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                int t = p[r][q];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
                if (lane == 0 && r < nr) S[(i64)q * G + g0 + r] = (((float)t * 0x1p-4f) * s_q[q]) * m;
            }
        }
    }
}

// =====================================================================================
// host drivers
// =====================================================================================
constexpr size_t FP4_GEMV_LDS = 64 * 1024;

// the planes of whole 128-row tiles, then s_q of those rows
static size_t fp4_planes_only(i64 Q, int ld) { return (size_t)cdiv(Q, 128) * 4 * (ld / 32) * 2048; }
static size_t fp4_planes_bytes(i64 Q, int D) { return fp4_planes_only(Q, fp4_ld(D)) + (size_t)cdiv(Q, 128) * 128 * sizeof(float); }
static bool fp4_gemv(i64 Q, int ld) { return Q <= 4 && (size_t)Q * 2 * ld <= FP4_GEMV_LDS; }

// qn [Q][dim] normalised -> planes and s_q in qs (fp4_planes_bytes(Q, dim))
static int split_queries_fp4(const float* qn, void* qs, i64 Q, int dim, int ld, hipStream_t st) {
    const int rows_pad = cdiv(Q, 128) * 128;
    unsigned char* planes = (unsigned char*)qs;
    hipLaunchKernelGGL(k_split_queries_fp4, dim3((unsigned)cdiv(rows_pad, 4)), dim3(256), 0, st, qn, planes,
                       reinterpret_cast<float*>(planes + fp4_planes_only(Q, ld)), (int)Q, dim, ld / 32, rows_pad, vec_ok(qn, dim));
    MI355_LAUNCH_CHECK();
    return OK;
}

// The fp4 row kind of RowsGemm and rank_topk_rows (rows_gemm.h).  TileArgs: qry = the queries' planes with s_q behind them,
// ginv = the rows' multipliers, D = ld.  The GEMV reads the GEMM's planes, so every search carves them and splits the queries
// first.
struct Fp4Rows {
    static constexpr bool SCALED = true, GEMV_PLANES = true;
    static constexpr int MAX_DIM = FP4_MAX_DIM, PATH_GEMV = MI355_RANK_PATH_FP4_GEMV;
    static constexpr const char* GEMV_RANGE = "rank/cosine gemv (fp4 gallery)";
    static constexpr const char* GEMM_RANGE = "rank/cosine gemm (fp4 gallery)";
    static constexpr const char* SELECT_RANGE = "rank/cosine gemm (fp4 gallery) + per-tile top-k";
    static constexpr auto ld = fp4_ld;
    static constexpr auto planes_bytes = fp4_planes_bytes;
    static constexpr auto gemv = fp4_gemv;
    template <int MT, int FK> static constexpr auto plain_kernel() { return &k_cos_gemm_fp4<MT, FK>; }
    template <int MT, class Epi> static constexpr auto epi_kernel() { return &k_cos_gemm_fp4_epi<MT, Epi>; }
    template <class K, class Epi>
    static void launch(K kernel, dim3 grid, size_t lds, hipStream_t st, const TileArgs& a, const Epi& epi, int x0, int ntx, int xtiles,
                       int ny) {
        const unsigned char* qs = (const unsigned char*)a.qry;
        const float* sq = reinterpret_cast<const float*>(qs + fp4_planes_only(a.Q, a.D));
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, qs, sq, (const unsigned char*)a.gal, a.ginv, a.Q, a.G, a.D, x0, ntx, xtiles,
                           ny, epi);
    }
    template <int NQ>
    static int gemv_launch(const RankWs& w, const void* codes, const float* mults, i64 G, int dim, int ld, unsigned blocks,
                           hipStream_t st) {
        if (int e = split_queries_fp4(w.qn, w.qs, NQ, dim, ld, st)) return e;
        const unsigned char* qs = (const unsigned char*)w.qs;
        const float* sq = reinterpret_cast<const float*>(qs + fp4_planes_only(NQ, ld));
        hipLaunchKernelGGL((k_cos_gemv_fp4<NQ>), dim3(blocks), dim3(256), (size_t)NQ * 2 * ld, st, qs, sq, (const unsigned char*)codes,
                           mults, w.S, G, ld);
        return OK;
    }
    template <class Epi>
    static int cos_gemm(const void* codes, const float* mults, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                        hipStream_t st) {
        return cos_gemm_fp4(codes, mults, ld, qn, qs, Q, G, dim, epi, st);
    }
};

template <class Epi>
int cos_gemm_fp4(const void* codes, const float* mults, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                 hipStream_t st) {
    set_rank_path(MI355_RANK_PATH_FP4_GEMM | (is_select<Epi> ? MI355_RANK_PATH_FUSED : 0));
    if (int e = split_queries_fp4(qn, qs, Q, dim, ld, st)) return e;
    return cos_gemm_tiles<RowsGemm<Fp4Rows>>({qs, codes, mults, (int)Q, G, ld}, epi, st);
}
template int cos_gemm_fp4(const void*, const float*, int, const float*, void*, i64, i64, int, const RangeArgs&, hipStream_t);

static GalleryRows fp4_rows(const void* codes, const float* mults, int dim) {
    GalleryRows g{nullptr, true, nullptr, fp4_ld(dim), fp4_planes_bytes};
    g.scales = mults;
    g.fp4 = codes;
    return g;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_gallery_fp4_bytes(int64_t G, int dim) {
    if (G < 0 || dim < 1) return 0;
    return (size_t)G * fp4_ld(dim);
}

int mi355_gallery_to_fp4(const float* rows, int64_t G, int dim, int rows_are_normalized, float eps, void* codes, size_t codes_bytes,
                         float* mults, void* stream) {
    MI355_REQUIRE(rows && codes && mults, "gallery_to_fp4: null pointer");
    MI355_REQUIRE(G >= 0 && dim >= 1, "gallery_to_fp4: bad shape G=%lld dim=%d", (long long)G, dim);
    MI355_REQUIRE(dim <= FP4_MAX_DIM, "gallery_to_fp4: dim=%d exceeds %d", dim, FP4_MAX_DIM);
    MI355_REQUIRE(((uintptr_t)codes & 15) == 0, "gallery_to_fp4: output buffer must be 16-byte aligned");
    MI355_REQUIRE(codes_bytes >= mi355_gallery_fp4_bytes(G, dim), "gallery_to_fp4: output buffer %zu < %zu bytes", codes_bytes,
                  mi355_gallery_fp4_bytes(G, dim));
    if (G == 0) return OK;
    hipLaunchKernelGGL(k_rows_to_fp4, dim3((unsigned)cdiv(G, 4)), dim3(256), 0, (hipStream_t)stream, rows, (unsigned char*)codes, mults,
                       (i64)G, dim, fp4_ld(dim), eps, rows_are_normalized ? 0 : 1, vec_ok(rows, dim));
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t mi355_rank_fp4_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || G < 1 || dim < 1 || dim > FP4_MAX_DIM || k < 1 || k > LARGE_K) return 0;
    return carve(nullptr, Q, G, dim, k, fp4_planes_bytes, false).total;
}

int mi355_rank_topk_fp4(const float* queries, int64_t Q, const void* codes, const float* mults, int64_t G, int dim, int k, float eps,
                        int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_topk_rows<Fp4Rows>(queries, Q, codes, mults, G, dim, k, eps, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                                   stream, nullptr, "rank_topk_fp4");
}

int mi355_rank_topk_fp4_filtered(const float* queries, int64_t Q, const void* codes, const float* mults, int64_t G, int dim, int k,
                                 float eps, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(filter, "rank_topk_fp4_filtered: null filter (use the unfiltered entry)");
    return rank_topk_rows<Fp4Rows>(queries, Q, codes, mults, G, dim, k, eps, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                                   stream, filter, "rank_topk_fp4_filtered");
}

size_t mi355_range_fp4_workspace_bytes(int64_t Q, int64_t G, int dim) {
    if (Q < 0 || G < 0 || dim < 1 || dim > FP4_MAX_DIM) return 0;
    return range_carve(nullptr, Q, G, dim, fp4_planes_bytes, false).total;   // normalised queries + one call's planes + table
}

int mi355_cosine_range_fp4(const float* queries, int64_t Q, const void* codes, const float* mults, int64_t G, int dim, float eps,
                           double threshold, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity,
                           int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(dim <= FP4_MAX_DIM, "cosine_range_fp4: dim=%d exceeds %d", dim, FP4_MAX_DIM);
    MI355_REQUIRE(mults || !codes, "cosine_range_fp4: null queries/gallery pointer");
    return cosine_range(queries, Q, fp4_rows(codes, mults, dim), G, dim, eps, threshold, idx_offset, filter, candidates, capacity, nnz,
                        workspace, workspace_bytes, stream, false, "cosine_range_fp4");
}

}  // extern "C"
