// 8-bit resident gallery: scalar-quantised int8 rows with one fp32 scale per row, and the cosine / top-k / range search over
// them on v_mfma_i32_32x32x32_i8.  gfx950 only.
//
// Numerical contract (include/mi355_retrieval.h).  "fp32" = one IEEE rounding per named operation.
//   * row quantiser (gallery rows and the query's hi plane): n = the fp32 row mi355_l2_normalize_rows writes for x (one shared
//     norm, row_inv_norm, same vec rule), amax = max |n_i|.  A NaN element or a non-finite amax: scale = NaN, codes 0.
//     amax < 1e-30: scale = 0, codes 0.  Else scale = amax / 127, inv = 127 / amax, code_i = clamp(rintf(n_i * inv), -127, 127)
//     (round-half-even).  Codes are int8, ld = dim rounded up to a multiple of 128 bytes per row, bytes dim .. ld-1 zero; the
//     scales are an fp32 array [G] beside them.
//   * query planes, per call, from qn = l2_normalize_rows(q): (hi, s_q) = the row quantiser of qn, r_i = fmaf(-hi_i, s_q, qn_i),
//     lo_i = clamp(rintf(r_i * (128 / s_q)), -127, 127) (|lo_i| <= 64; lo = 0 when s_q is 0 or NaN): about 15 bits of the query.
//   * score: acc_hi = sum hi_i c_i, acc_lo = sum lo_i c_i, exact in int32 (dim <= 65536); t = fmaf(float(acc_lo), 2^-7,
//     float(acc_hi)); score = (t * s_q) * s_g.  A NaN row scores NaN, a zero row 0, a NaN query NaN everywhere.
//   * the integer sums do not depend on any summation order, so the GEMV (Q <= 4), both tile sizes of the GEMM, its two
//     launches and every epilogue return the SAME bits for a (query, row) pair.
//   * order, ties, NaN, pads: the selection of mi355_rank_topk (rank_common.h).
#include "i8_quant.h"
#include "rows_gemm.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef int i32x16 __attribute__((ext_vector_type(16)));

// =====================================================================================
// fp32 rows -> int8 codes, padded to ld bytes with zeros, and one scale per row.  One wave per row: the norm with
// row_inv_norm, amax by wave reduction, then the codes.  Appendable: converting n rows to codes + r * ld, scales + r writes
// rows r .. r+n-1.
// =====================================================================================
__global__ __launch_bounds__(256) void k_rows_to_i8(const float* __restrict__ in, signed char* __restrict__ codes,
                                                    float* __restrict__ scales, i64 rows, int dim, int ld, float eps,
                                                    int normalize, int vec) {
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = in + row * dim;
    const float r = normalize ? row_inv_norm(x, dim, eps, vec, lane) : 1.0f;
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
    const I8Quant q = i8_quant(wave_max(amax), __ballot(nan) != 0ull);
    if (lane == 0) scales[row] = q.scale;
    signed char* y = codes + row * ld;
    if (vec) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        for (int i = lane; i < ld / 4; i += 64) {
            unsigned w = 0u;
            if (i < dim / 4 && !q.zero) {
                const f32x4 v = x4[i];
                w = pack4_i8(i8_code(i8_norm_elem(v.x, r), q.inv), i8_code(i8_norm_elem(v.y, r), q.inv),
                             i8_code(i8_norm_elem(v.z, r), q.inv), i8_code(i8_norm_elem(v.w, r), q.inv));
            }
            reinterpret_cast<unsigned*>(y)[i] = w;
        }
    } else {
        for (int i = lane; i < ld; i += 64) y[i] = (i < dim && !q.zero) ? (signed char)i8_code(i8_norm_elem(x[i], r), q.inv) : (signed char)0;
    }
}

// =====================================================================================
// Normalised queries -> their two int8 planes in MFMA-fragment order and s_q per query:
// Qs[row block of 32][k sub-step of 32][plane hi, lo][lane][16 B], lane = row + 32 * (k half): the lane's 16 bytes are the 16
// consecutive k of its half of the sub-step.  A GEMM k-step of 128 is then 8 KB per row block, eight 1 KB pieces that LDS-DMA
// moves as they are.  One wave per row of the rows_pad (whole 128-row tiles) rows; rows >= Q and k >= D are zero, sq 0.
// =====================================================================================
__global__ __launch_bounds__(256) void k_split_queries_i8(const float* __restrict__ Qn, signed char* __restrict__ Qs,
                                                          float* __restrict__ sq, int Q, int D, int n_sub, int rows_pad,
                                                          int vec) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_pad) return;
    const float* x = Qn + (i64)row * D;
    I8Quant q = {0.f, 0.f, true};
    if (row < Q) {
        float amax = 0.f;
        bool nan = false;
        if (vec) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
            for (int i = lane; i < D / 4; i += 64) {
                const f32x4 v = x4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    nan = nan || v[e] != v[e];
                    amax = fmaxf(amax, fabsf(v[e]));
                }
            }
        } else {
            for (int i = lane; i < D; i += 64) {
                const float n = x[i];
                nan = nan || n != n;
                amax = fmaxf(amax, fabsf(n));
            }
        }
        q = i8_quant(wave_max(amax), __ballot(nan) != 0ull);
    }
    if (lane == 0) sq[row] = q.scale;
    const float lo_mul = i8_lo_mul(q);
    signed char* base = Qs + (size_t)(row >> 5) * n_sub * 2048 + (row & 31) * 16;
    for (int c = lane; c < 2 * n_sub; c += 64) {           // 16-byte chunk c: sub-step c / 2, k half c % 2
        unsigned hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
        if (!q.zero) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int k0 = c * 16 + w * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (vec) {                                 // D % 4 == 0: a group of four lies inside the row or past it
                    if (k0 < D) v = *reinterpret_cast<const f32x4*>(x + k0);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = k0 + e < D ? x[k0 + e] : 0.f;
                }
                int h[4], l[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) i8_split_elem(v[e], q, lo_mul, h[e], l[e]);
                hi[w] = pack4_i8(h[0], h[1], h[2], h[3]);
                lo[w] = pack4_i8(l[0], l[1], l[2], l[3]);
            }
        }
        signed char* o = base + (size_t)(c >> 1) * 2048 + (c & 1) * 512;
        *reinterpret_cast<i32x4*>(o) = (i32x4){(int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        *reinterpret_cast<i32x4*>(o + 1024) = (i32x4){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3]};
    }
}

// =====================================================================================
// cosine GEMM over int8 rows: the DMA-ring loop of rows_gemm.h with 16 codes per fragment on v_mfma_i32_32x32x32_i8 (a sub-step
// is 32 k), int32 accumulators, and the float tail t = fmaf(float(acc_lo), 2^-7, float(acc_hi)), then t * s_q per accumulator
// row; the epilogue's acc * ginv[col] is the multiply by s_g.  (sq holds whole 128-row tiles: rows >= Q read 0.)
// Fragment map: a lane's A and B fragments of a sub-step are the SAME 16 consecutive k (its half of the sub-step), byte for
// byte.  The MFMA pairs A and B bytes by (lane half, byte), and an integer sum does not depend on the k order, so whichever k
// the hardware calls them the result is the exact dot product.
// =====================================================================================
struct I8Tile {
    typedef i32x4 Frag;
    typedef i32x16 Acc;
    const float* __restrict__ sq;       // s_q of the call's queries
    const float* __restrict__ scales;   // s_g of the gallery rows
    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0); }
    __device__ __forceinline__ void tail(const Acc (&hi)[2], const Acc (&lo)[2], f32x16 (&acc)[2], int row0, int lane) const {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = sq[row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j][r] = __builtin_fmaf((float)lo[j][r], 0x1p-7f, (float)hi[j][r]) * s;
        }
    }
    __device__ __forceinline__ const float* ginv() const { return scales; }
};
static_assert(I8_KSTEP == ROWS_KSTEP, "a k-step is one 128-byte segment of a stored row");

template <int MT, int FK>
__global__ __launch_bounds__(256) void k_cos_gemm_i8(const signed char* __restrict__ Qs, const float* __restrict__ sq,
                                                     const signed char* __restrict__ Gal, const float* __restrict__ scales, int Q,
                                                     i64 G, int ld, int x0, int ntx, int xtiles, int ny, PlainEpi<FK> epi) {
    rows_gemm_tile<I8Tile, MT>((const char*)Qs, (const char*)Gal, I8Tile{sq, scales}, Q, G, ld, x0, ntx, xtiles, ny, epi);
}
// Every other epilogue (filtered selection, range): the same loop
template <int MT, class Epi>
__global__ __launch_bounds__(256) void k_cos_gemm_i8_epi(const signed char* __restrict__ Qs, const float* __restrict__ sq,
                                                         const signed char* __restrict__ Gal, const float* __restrict__ scales,
                                                         int Q, i64 G, int ld, int x0, int ntx, int xtiles, int ny, Epi epi) {
    rows_gemm_tile<I8Tile, MT>((const char*)Qs, (const char*)Gal, I8Tile{sq, scales}, Q, G, ld, x0, ntx, xtiles, ny, epi);
}

// =====================================================================================
// Few queries (Q <= 4, the one-query-at-a-time serving shape): a GEMV bound by streaming the gallery once (ld bytes per
// row).  One wave per row, 16 bytes per lane per load, up to four loads in flight per lane; the queries' two int8 planes (the
// ones the GEMM reads, taken out of their fragment order) sit in LDS as [NQ][hi, lo][ld].  Integer dot products, reduced over
// the wave in integers, then the float tail of the GEMM: the same bits.
// =====================================================================================
template <int NQ>
__global__ __launch_bounds__(256) void k_cos_gemv_i8(const signed char* __restrict__ Qs, const float* __restrict__ sq,
                                                     const signed char* __restrict__ Gal, const float* __restrict__ scales,
                                                     float* __restrict__ S, i64 G, int ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    i32x4* qs = reinterpret_cast<i32x4*>(smem);                  // [NQ][2][ld / 16] chunks
    const int nch = ld / 16;                                     // 16-byte chunks per row
    for (int i = threadIdx.x; i < NQ * 2 * nch; i += 256) {
        const int q = i / (2 * nch), p = (i / nch) & 1, c = i % nch;
        qs[i] = *reinterpret_cast<const i32x4*>(Qs + ((size_t)((c >> 1) * 2 + p) * 64 + (c & 1) * 32 + q) * 16);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const i64 wave_id = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const i64 nwaves = (i64)gridDim.x * 4;
    float s_q[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) s_q[q] = sq[q];
    for (i64 g = wave_id; g < G; g += nwaves) {
        const i32x4* row = reinterpret_cast<const i32x4*>(Gal + g * ld);
        int hi[NQ], lo[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { hi[q] = 0; lo[q] = 0; }
        for (int c0 = 0; c0 < nch; c0 += 4 * 64) {
            i32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                v[u] = c < nch ? row[c] : (i32x4){0, 0, 0, 0};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                if (c < nch) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const i32x4 h = qs[(q * 2) * nch + c], l = qs[(q * 2 + 1) * nch + c];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            hi[q] = __builtin_amdgcn_sdot4(h[e], v[u][e], hi[q], false);
                            lo[q] = __builtin_amdgcn_sdot4(l[e], v[u][e], lo[q], false);
                        }
                    }
                }
            }
        }
        const float s_g = scales[g];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            int h = hi[q], l = lo[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { h += __shfl_xor(h, o, 64); l += __shfl_xor(l, o, 64); }
            if (lane == 0) S[(i64)q * G + g] = (__builtin_fmaf((float)l, 0x1p-7f, (float)h) * s_q[q]) * s_g;
        }
    }
}

// =====================================================================================
// host drivers
// =====================================================================================
constexpr size_t I8_GEMV_LDS = 64 * 1024;

// the planes of whole 128-row tiles, then s_q of those rows
static size_t i8_planes_only(i64 Q, int ld) { return (size_t)cdiv(Q, 128) * 4 * (ld / 32) * 2048; }
static size_t i8_planes_bytes(i64 Q, int D) { return i8_planes_only(Q, i8_ld(D)) + (size_t)cdiv(Q, 128) * 128 * sizeof(float); }
static bool i8_gemv(i64 Q, int ld) { return Q <= 4 && (size_t)Q * 2 * ld <= I8_GEMV_LDS; }

// qn [Q][dim] normalised -> planes and s_q in qs (i8_planes_bytes(Q, dim))
static int split_queries_i8(const float* qn, void* qs, i64 Q, int dim, int ld, hipStream_t st) {
    const int rows_pad = cdiv(Q, 128) * 128;
    signed char* planes = (signed char*)qs;
    hipLaunchKernelGGL(k_split_queries_i8, dim3((unsigned)cdiv(rows_pad, 4)), dim3(256), 0, st, qn, planes,
                       reinterpret_cast<float*>(planes + i8_planes_only(Q, ld)), (int)Q, dim, ld / 32, rows_pad, vec_ok(qn, dim));
    MI355_LAUNCH_CHECK();
    return OK;
}

// The int8 row kind of RowsGemm and rank_topk_rows (rows_gemm.h).  TileArgs: qry = the queries' planes with s_q behind them,
// ginv = the rows' scales, D = ld.  The GEMV reads the GEMM's planes, so every search carves them and splits the queries first.
struct I8Rows {
    static constexpr bool SCALED = true, GEMV_PLANES = true;
    static constexpr int MAX_DIM = I8_MAX_DIM, PATH_GEMV = MI355_RANK_PATH_I8_GEMV;
    static constexpr const char* GEMV_RANGE = "rank/cosine gemv (int8 gallery)";
    static constexpr const char* GEMM_RANGE = "rank/cosine gemm (int8 gallery)";
    static constexpr const char* SELECT_RANGE = "rank/cosine gemm (int8 gallery) + per-tile top-k";
    static constexpr auto ld = i8_ld;
    static constexpr auto planes_bytes = i8_planes_bytes;
    static constexpr auto gemv = i8_gemv;
    template <int MT, int FK> static constexpr auto plain_kernel() { return &k_cos_gemm_i8<MT, FK>; }
    template <int MT, class Epi> static constexpr auto epi_kernel() { return &k_cos_gemm_i8_epi<MT, Epi>; }
    template <class K, class Epi>
    static void launch(K kernel, dim3 grid, size_t lds, hipStream_t st, const TileArgs& a, const Epi& epi, int x0, int ntx, int xtiles,
                       int ny) {
        const signed char* qs = (const signed char*)a.qry;
        const float* sq = reinterpret_cast<const float*>(qs + i8_planes_only(a.Q, a.D));
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, qs, sq, (const signed char*)a.gal, a.ginv, a.Q, a.G, a.D, x0, ntx, xtiles,
                           ny, epi);
    }
    template <int NQ>
    static int gemv_launch(const RankWs& w, const void* codes, const float* scales, i64 G, int dim, int ld, unsigned blocks,
                           hipStream_t st) {
        if (int e = split_queries_i8(w.qn, w.qs, NQ, dim, ld, st)) return e;
        const signed char* qs = (const signed char*)w.qs;
        const float* sq = reinterpret_cast<const float*>(qs + i8_planes_only(NQ, ld));
        hipLaunchKernelGGL((k_cos_gemv_i8<NQ>), dim3(blocks), dim3(256), (size_t)NQ * 2 * ld, st, qs, sq, (const signed char*)codes, scales,
                           w.S, G, ld);
        return OK;
    }
    template <class Epi>
    static int cos_gemm(const void* codes, const float* scales, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                        hipStream_t st) {
        return cos_gemm_i8(codes, scales, ld, qn, qs, Q, G, dim, epi, st);
    }
};

template <class Epi>
int cos_gemm_i8(const void* codes, const float* scales, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                hipStream_t st) {
    set_rank_path(MI355_RANK_PATH_I8_GEMM | (is_select<Epi> ? MI355_RANK_PATH_FUSED : 0));
    if (int e = split_queries_i8(qn, qs, Q, dim, ld, st)) return e;
    return cos_gemm_tiles<RowsGemm<I8Rows>>({qs, codes, scales, (int)Q, G, ld}, epi, st);
}
template int cos_gemm_i8(const void*, const float*, int, const float*, void*, i64, i64, int, const RangeArgs&, hipStream_t);

static GalleryRows i8_rows(const void* codes, const float* scales, int dim) {
    return {nullptr, true, nullptr, i8_ld(dim), i8_planes_bytes, codes, scales};
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_gallery_i8_bytes(int64_t G, int dim) {
    if (G < 0 || dim < 1) return 0;
    return (size_t)G * i8_ld(dim);
}

int mi355_gallery_to_i8(const float* rows, int64_t G, int dim, int rows_are_normalized, float eps, void* codes, size_t codes_bytes,
                        float* scales, void* stream) {
    MI355_REQUIRE(rows && codes && scales, "gallery_to_i8: null pointer");
    MI355_REQUIRE(G >= 0 && dim >= 1, "gallery_to_i8: bad shape G=%lld dim=%d", (long long)G, dim);
    MI355_REQUIRE(dim <= I8_MAX_DIM, "gallery_to_i8: dim=%d exceeds %d", dim, I8_MAX_DIM);
    MI355_REQUIRE(((uintptr_t)codes & 15) == 0, "gallery_to_i8: output buffer must be 16-byte aligned");
    MI355_REQUIRE(codes_bytes >= mi355_gallery_i8_bytes(G, dim), "gallery_to_i8: output buffer %zu < %zu bytes", codes_bytes,
                  mi355_gallery_i8_bytes(G, dim));
    if (G == 0) return OK;
    hipLaunchKernelGGL(k_rows_to_i8, dim3((unsigned)cdiv(G, 4)), dim3(256), 0, (hipStream_t)stream, rows, (signed char*)codes, scales,
                       (i64)G, dim, i8_ld(dim), eps, rows_are_normalized ? 0 : 1, vec_ok(rows, dim));
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t mi355_rank_i8_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || G < 1 || dim < 1 || dim > I8_MAX_DIM || k < 1 || k > LARGE_K) return 0;
    return carve(nullptr, Q, G, dim, k, i8_planes_bytes, false).total;
}

int mi355_rank_topk_i8(const float* queries, int64_t Q, const void* codes, const float* scales, int64_t G, int dim, int k, float eps,
                       int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_topk_rows<I8Rows>(queries, Q, codes, scales, G, dim, k, eps, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                                  stream, nullptr, "rank_topk_i8");
}

int mi355_rank_topk_i8_filtered(const float* queries, int64_t Q, const void* codes, const float* scales, int64_t G, int dim, int k,
                                float eps, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                                void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(filter, "rank_topk_i8_filtered: null filter (use the unfiltered entry)");
    return rank_topk_rows<I8Rows>(queries, Q, codes, scales, G, dim, k, eps, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                                  stream, filter, "rank_topk_i8_filtered");
}

size_t mi355_range_i8_workspace_bytes(int64_t Q, int64_t G, int dim) {
    if (Q < 0 || G < 0 || dim < 1 || dim > I8_MAX_DIM) return 0;
    return range_carve(nullptr, Q, G, dim, i8_planes_bytes, false).total;   // normalised queries + one call's planes + table
}

int mi355_cosine_range_i8(const float* queries, int64_t Q, const void* codes, const float* scales, int64_t G, int dim, float eps,
                          double threshold, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity,
                          int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(dim <= I8_MAX_DIM, "cosine_range_i8: dim=%d exceeds %d", dim, I8_MAX_DIM);
    MI355_REQUIRE(scales || !codes, "cosine_range_i8: null queries/gallery pointer");
    return cosine_range(queries, Q, i8_rows(codes, scales, dim), G, dim, eps, threshold, idx_offset, filter, candidates, capacity, nnz,
                        workspace, workspace_bytes, stream, false, "cosine_range_i8");
}

}  // extern "C"
