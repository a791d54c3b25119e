// Half-precision resident gallery: fp16 rows and the cosine / top-k search over them.  gfx950 only.
//
// Numerical contract (include/mi355_retrieval.h):
//   * stored row = fp16_rne(l2_normalize_rows(x, eps)) - the same fp32 row mi355_l2_normalize_rows writes (one shared norm,
//     row_inv_norm), rounded once to nearest-even; it is not renormalised after rounding.  Rows are padded with zeros to a
//     stride of a multiple of 64 elements (128 B), so that every load of the search is a whole 128-byte row segment.
//   * score = qn . float(row), qn the query normalised as mi355_rank_topk normalises it.  The GEMM (Q > 4) carries qn as two
//     fp16 planes, hi = fp16(qn) and lo = fp16((qn - hi) * 2^11) (22 significant bits), multiplies each with the stored row
//     on v_mfma_f32_32x32x16_f16 into its own fp32 accumulator (every fp16 x fp16 product is exact in fp32) and returns
//     acc_hi + acc_lo * 2^-11.  The GEMV (Q <= 4) uses the fp32 qn directly.  Either way |score - qn . row| stays ~1e-7.
//   * order, ties, NaN: the selection of mi355_rank_topk (rank_common.h), so the same rule as cosine_topk / torch.topk.
#include "rows_gemm.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef _Float16 f16;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int F16_KSTEP = 64;                 // k-step of the GEMM: one 128-byte segment of a stored row
static inline int f16_ld(int dim) { return (dim + F16_KSTEP - 1) / F16_KSTEP * F16_KSTEP; }

// =====================================================================================
// fp32 rows -> normalised fp16 rows, padded to ld elements with zeros.  One wave per row; the norm is row_inv_norm (the
// one mi355_l2_normalize_rows uses, with the same vec rule), so the stored row is bit for bit l2_normalize_rows(x).half().
// =====================================================================================
__global__ __launch_bounds__(256) void k_rows_to_f16(const float* __restrict__ in, f16* __restrict__ out, i64 rows, int dim,
                                                     int ld, float eps, int normalize, int vec) {
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = in + row * dim;
    const float r = normalize ? row_inv_norm(x, dim, eps, vec, lane) : 1.0f;
    f16* y = out + row * ld;
    if (vec) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        for (int i = lane; i < ld / 4; i += 64) {
            f16x4 h = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
            if (i < dim / 4) {
                const f32x4 v = x4[i];
                h = (f16x4){scaled_f16(v.x, r), scaled_f16(v.y, r), scaled_f16(v.z, r), scaled_f16(v.w, r)};
            }
            reinterpret_cast<f16x4*>(y)[i] = h;
        }
    } else {
        for (int i = lane; i < ld; i += 64) y[i] = i < dim ? scaled_f16(x[i], r) : (f16)0.f;
    }
}

// =====================================================================================
// Normalised queries -> the two fp16 planes in MFMA-fragment order: Qs[row block of 32][k sub-step of 16][plane hi, lo]
// [lane][8 f16], lane = row + 32 * (k half), as k_split_queries lays out its bf16 planes.  A GEMM k-step of 64 is then
// 8 KB per row block, eight 1 KB pieces that LDS-DMA moves as they are.  Rows >= Q and k >= D are zero.
// =====================================================================================
constexpr float F16_LO_SCALE = 2048.0f;       // 2^11: the lo plane (|qn - hi| <= 2^-11 |qn|) stays in fp16's normal range
constexpr float F16_LO_UNSCALE = 1.0f / 2048.0f;

__global__ __launch_bounds__(256) void k_split_queries_f16(const float* __restrict__ Qn, f16* __restrict__ Qs, int Q, int D,
                                                           int n_sub, int n_frag) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);   // fragment = (row block, k sub-step)
    if (f >= n_frag) return;
    const int lane = threadIdx.x & 63;
    const int rb = f / n_sub, s = f % n_sub;
    const int row = rb * 32 + (lane & 31), k0 = s * 16 + (lane >> 5) * 8;
    f16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (row < Q && k0 + e < D) ? Qn[(i64)row * D + k0 + e] : 0.f;
        const f16 h = (f16)x;
        hi[e] = h;
        lo[e] = (f16)((x - (float)h) * F16_LO_SCALE);   // x - h is exact in fp32, the scale by 2^11 too
    }
    f16x8* o = reinterpret_cast<f16x8*>(Qs + (size_t)f * 2 * 512) + lane;
    o[0] = hi;
    o[64] = lo;
}

// =====================================================================================
// cosine GEMM over fp16 rows: the DMA-ring loop of rows_gemm.h with 8 f16 per fragment on v_mfma_f32_32x32x16_f16 (a sub-step
// is 16 k), fp32 accumulators, and the tail acc_hi + acc_lo * 2^-11.  The stored rows are unit length: no column scale.
// =====================================================================================
struct F16Tile {
    typedef f16x8 Frag;
    typedef f32x16 Acc;
    static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    __device__ __forceinline__ void tail(const Acc (&hi)[2], const Acc (&lo)[2], f32x16 (&acc)[2], int, int) const {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = __builtin_fmaf(lo[j][e], F16_LO_UNSCALE, hi[j][e]);
    }
    __device__ __forceinline__ const float* ginv() const { return nullptr; }
};
static_assert(F16_KSTEP * sizeof(f16) == ROWS_KSTEP, "a k-step is one 128-byte segment of a stored row");

template <int MT, int FK>
__global__ __launch_bounds__(256) void k_cos_gemm_f16(const f16* __restrict__ Qs, const f16* __restrict__ Gal, int Q, i64 G,
                                                      int ld, int x0, int ntx, int xtiles, int ny, PlainEpi<FK> epi) {
    rows_gemm_tile<F16Tile, MT>((const char*)Qs, (const char*)Gal, F16Tile{}, Q, G, ld * (int)sizeof(f16), x0, ntx, xtiles, ny, epi);
}
// Every other epilogue (filtered selection, histogram, range, ranks): the same loop
template <int MT, class Epi>
__global__ __launch_bounds__(256) void k_cos_gemm_f16_epi(const f16* __restrict__ Qs, const f16* __restrict__ Gal, int Q, i64 G,
                                                          int ld, int x0, int ntx, int xtiles, int ny, Epi epi) {
    rows_gemm_tile<F16Tile, MT>((const char*)Qs, (const char*)Gal, F16Tile{}, Q, G, ld * (int)sizeof(f16), x0, ntx, xtiles, ny, epi);
}

// =====================================================================================
// Few queries (Q <= 4, the one-query-at-a-time serving shape): a GEMV bound by streaming the gallery once (2 * ld bytes
// per row).  One wave per row, 16 bytes per lane per load, up to four loads in flight per lane; the fp32 queries sit in
// LDS, padded with zeros to ld.
// =====================================================================================
template <int NQ>
__global__ __launch_bounds__(256) void k_cos_gemv_f16(const float* __restrict__ Qn, const f16* __restrict__ Gal,
                                                      float* __restrict__ S, i64 G, int D, int ld) {
    extern __shared__ __attribute__((aligned(16))) float qs[];   // [NQ][ld]
    for (int i = threadIdx.x; i < NQ * ld; i += 256) {
        const int q = i / ld, e = i - q * ld;
        qs[i] = e < D ? Qn[(i64)q * D + e] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int nch = ld / 8;                                      // 16-byte chunks per row
    const i64 wave_id = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 g = wave_id; g < G; g += nwaves) {
        const f16x8* row = reinterpret_cast<const f16x8*>(Gal + g * ld);
        float acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
        for (int c0 = 0; c0 < nch; c0 += 4 * 64) {
            f16x8 h[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                h[u] = c < nch ? row[c] : (f16x8){};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                if (c < nch) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const f32x4 u0 = *reinterpret_cast<const f32x4*>(&qs[q * ld + c * 8]);
                        const f32x4 u1 = *reinterpret_cast<const f32x4*>(&qs[q * ld + c * 8 + 4]);
                        acc[q] += (float)h[u][0] * u0.x + (float)h[u][1] * u0.y + (float)h[u][2] * u0.z + (float)h[u][3] * u0.w +
                                  (float)h[u][4] * u1.x + (float)h[u][5] * u1.y + (float)h[u][6] * u1.z + (float)h[u][7] * u1.w;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float t = wave_sum(acc[q]);
            if (lane == 0) S[(i64)q * G + g] = t;
        }
    }
}

// =====================================================================================
// host drivers
// =====================================================================================
constexpr size_t F16_GEMV_LDS = 64 * 1024;

static size_t f16_planes_bytes(i64 Q, int D) { return (size_t)cdiv(Q, 128) * 4 * (f16_ld(D) / 16) * 2 * 1024; }
static bool f16_gemv(i64 Q, int ld) { return Q <= 4 && (size_t)Q * ld * sizeof(float) <= F16_GEMV_LDS; }

// The fp16 row kind of RowsGemm and rank_topk_rows (rows_gemm.h).  TileArgs::D is ld in f16 elements; the GEMV reads the fp32
// queries, so a search that takes it carves no planes.
struct F16Rows {
    static constexpr bool SCALED = false, GEMV_PLANES = false;
    static constexpr int MAX_DIM = 0, PATH_GEMV = MI355_RANK_PATH_F16_GEMV;
    static constexpr const char* GEMV_RANGE = "rank/cosine gemv (fp16 gallery)";
    static constexpr const char* GEMM_RANGE = "rank/cosine gemm (fp16 gallery)";
    static constexpr const char* SELECT_RANGE = "rank/cosine gemm (fp16 gallery) + per-tile top-k";
    static constexpr auto ld = f16_ld;
    static constexpr auto planes_bytes = f16_planes_bytes;
    static constexpr auto gemv = f16_gemv;
    template <int MT, int FK> static constexpr auto plain_kernel() { return &k_cos_gemm_f16<MT, FK>; }
    template <int MT, class Epi> static constexpr auto epi_kernel() { return &k_cos_gemm_f16_epi<MT, Epi>; }
    template <class K, class Epi>
    static void launch(K kernel, dim3 grid, size_t lds, hipStream_t st, const TileArgs& a, const Epi& epi, int x0, int ntx, int xtiles,
                       int ny) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, (const f16*)a.qry, (const f16*)a.gal, a.Q, a.G, a.D, x0, ntx, xtiles, ny, epi);
    }
    template <int NQ>
    static int gemv_launch(const RankWs& w, const void* rows, const float*, i64 G, int dim, int ld, unsigned blocks, hipStream_t st) {
        hipLaunchKernelGGL((k_cos_gemv_f16<NQ>), dim3(blocks), dim3(256), (size_t)NQ * ld * sizeof(float), st, w.qn, (const f16*)rows, w.S,
                           G, dim, ld);
        return OK;
    }
    template <class Epi>
    static int cos_gemm(const void* rows, const float*, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                        hipStream_t st) {
        return cos_gemm_f16(rows, ld, qn, qs, Q, G, dim, epi, st);
    }
};

template <class Epi>
int cos_gemm_f16(const void* rows, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi, hipStream_t st) {
    set_rank_path(MI355_RANK_PATH_F16_GEMM | (is_select<Epi> ? MI355_RANK_PATH_FUSED : 0));
    const int n_sub = ld / 16, n_frag = cdiv(Q, 128) * 4 * n_sub;
    hipLaunchKernelGGL(k_split_queries_f16, dim3((unsigned)cdiv(n_frag, 4)), dim3(256), 0, st, qn, (f16*)qs, (int)Q, dim, n_sub, n_frag);
    MI355_LAUNCH_CHECK();
    return cos_gemm_tiles<RowsGemm<F16Rows>>({qs, rows, nullptr, (int)Q, G, ld}, epi, st);
}
template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const RocArgs&, hipStream_t);
template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const RangeArgs&, hipStream_t);
template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const RanksArgs&, hipStream_t);
template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const NearestEpi&, hipStream_t);
template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const DegreeEpi&, hipStream_t);
template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const LinkEpi&, hipStream_t);
// the adjusted scores (adjusted_search, rank.hip): the slab and the fused selection with the map in front of it
template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const AdjSlabEpi&, hipStream_t);
#define ADJ_SELECT_F16(FK)                                                                                                  \
    template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const AdjSelectEpi<FK, false>&, hipStream_t); \
    template int cos_gemm_f16(const void*, int, const float*, void*, i64, i64, int, const AdjSelectEpi<FK, true>&, hipStream_t);
ADJ_SELECT_F16(1)
ADJ_SELECT_F16(2)
ADJ_SELECT_F16(4)
ADJ_SELECT_F16(8)
#undef ADJ_SELECT_F16

static GalleryRows f16_rows(const void* gallery_f16, int dim) { return {nullptr, true, gallery_f16, f16_ld(dim), f16_planes_bytes}; }

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_gallery_f16_bytes(int64_t G, int dim) {
    if (G < 0 || dim < 1) return 0;
    return (size_t)G * f16_ld(dim) * sizeof(f16);
}

int mi355_gallery_to_f16(const float* rows, int64_t G, int dim, int rows_are_normalized, float eps, void* out, size_t out_bytes,
                         void* stream) {
    MI355_REQUIRE(rows && out, "gallery_to_f16: null pointer");
    MI355_REQUIRE(G >= 0 && dim >= 1, "gallery_to_f16: bad shape G=%lld dim=%d", (long long)G, dim);
    MI355_REQUIRE(((uintptr_t)out & 15) == 0, "gallery_to_f16: output buffer must be 16-byte aligned");
    MI355_REQUIRE(out_bytes >= mi355_gallery_f16_bytes(G, dim), "gallery_to_f16: output buffer %zu < %zu bytes", out_bytes,
                  mi355_gallery_f16_bytes(G, dim));
    if (G == 0) return OK;
    hipLaunchKernelGGL(k_rows_to_f16, dim3((unsigned)cdiv(G, 4)), dim3(256), 0, (hipStream_t)stream, rows, (f16*)out, (i64)G, dim,
                       f16_ld(dim), eps, rows_are_normalized ? 0 : 1, vec_ok(rows, dim));
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t mi355_rank_f16_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || G < 1 || dim < 1 || k < 1 || k > LARGE_K) return 0;
    return carve(nullptr, Q, G, dim, k, f16_gemv(Q, f16_ld(dim)) ? nullptr : f16_planes_bytes, false).total;
}

int mi355_rank_topk_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, int k, float eps,
                        int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                        void* stream) {
    return rank_topk_rows<F16Rows>(queries, Q, gallery_f16, nullptr, G, dim, k, eps, idx_offset, out_val, out_idx, workspace,
                                   workspace_bytes, stream, nullptr, "rank_topk_f16");
}

int mi355_rank_topk_f16_filtered(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, int k, float eps,
                                 int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(filter, "rank_topk_f16_filtered: null filter (use the unfiltered entry)");
    return rank_topk_rows<F16Rows>(queries, Q, gallery_f16, nullptr, G, dim, k, eps, idx_offset, out_val, out_idx, workspace,
                                   workspace_bytes, stream, filter, "rank_topk_f16_filtered");
}

size_t mi355_rank_adjusted_f16_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || G < 1 || dim < 1 || k < 0 || k > LARGE_K) return 0;
    return carve(nullptr, Q, G, dim, k, f16_planes_bytes, false, k > 0).total;   // (no GEMV: the planes at every Q)
}

int mi355_rank_topk_adjusted_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, int k, float eps,
                                 int64_t idx_offset, const mi355_score_adjust* adjust, const mi355_rank_filter* filter,
                                 int64_t query_block, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    const GalleryRows g = f16_rows(gallery_f16, dim < 1 ? 1 : dim);
    ScoreAdjust adj{};
    RankFilter f{};
    if (int e = adjust_check(queries, Q, g, G, dim, k, true, adjust, filter, idx_offset, query_block, out_val, out_idx,
                             "rank_topk_adjusted_f16", &adj, &f))
        return e;
    if (Q == 0) return OK;
    return adjusted_search(queries, Q, g, G, dim, eps, k, idx_offset, adj, filter ? &f : nullptr, query_block, out_val, (i64*)out_idx,
                           workspace, workspace_bytes, (hipStream_t)stream, "rank_topk_adjusted_f16");
}

int mi355_cosine_scores_adjusted_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                                     const mi355_score_adjust* adjust, int64_t query_block, float* out, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const GalleryRows g = f16_rows(gallery_f16, dim < 1 ? 1 : dim);
    ScoreAdjust adj{};
    if (int e = adjust_check(queries, Q, g, G, dim, 0, false, adjust, nullptr, 0, query_block, out, nullptr,
                             "cosine_scores_adjusted_f16", &adj, nullptr))
        return e;
    if (Q == 0) return OK;
    return adjusted_search(queries, Q, g, G, dim, eps, 0, 0, adj, nullptr, query_block, out, nullptr, workspace, workspace_bytes,
                           (hipStream_t)stream, "cosine_scores_adjusted_f16");
}

size_t mi355_roc_pairs_f16_workspace_bytes(int64_t Q, int64_t G, int dim) {
    if (Q < 1 || G < 1 || dim < 1) return 0;
    return carve(nullptr, Q, G, dim, 0, f16_planes_bytes, false, false).total;   // normalised queries + one call's planes
}

int mi355_roc_pairs_hist_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                             const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude, int64_t idx_offset,
                             const double* thresholds, const double* thresholds_dev, int T, int64_t* hist, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return roc_pairs_hist(queries, Q, f16_rows(gallery_f16, dim), G, dim, eps, query_labels, gallery_labels, exclude, idx_offset,
                          thresholds, thresholds_dev, T, hist, workspace, workspace_bytes, mi355_roc_pairs_f16_workspace_bytes(Q, G, dim),
                          stream, "roc_pairs_hist_f16");
}

size_t mi355_range_f16_workspace_bytes(int64_t Q, int64_t G, int dim) {
    if (Q < 0 || G < 0 || dim < 1) return 0;
    return range_carve(nullptr, Q, G, dim, f16_planes_bytes, false).total;   // normalised queries + one call's planes + table
}

int mi355_cosine_range_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps, double threshold,
                           int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity, int64_t* nnz,
                           void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_range(queries, Q, f16_rows(gallery_f16, dim), G, dim, eps, threshold, idx_offset, filter, candidates, capacity, nnz,
                        workspace, workspace_bytes, stream, false, "cosine_range_f16");
}

int mi355_positives_range_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                              int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity, int64_t* nnz,
                              void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(filter && filter->label_mode == MI355_LABEL_SAME, "positives_range_f16: needs a filter with MI355_LABEL_SAME");
    return cosine_range(queries, Q, f16_rows(gallery_f16, dim), G, dim, eps, 0.0, idx_offset, filter, candidates, capacity, nnz,
                        workspace, workspace_bytes, stream, true, "positives_range_f16");
}

size_t mi355_rank_positives_f16_workspace_bytes(int64_t Q, int64_t G, int dim) {
    return mi355_roc_pairs_f16_workspace_bytes(Q, G, dim);
}

int mi355_rank_positives_f16(const float* queries, int64_t Q, const void* gallery_f16, int64_t G, int dim, float eps,
                             const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude, int64_t idx_offset,
                             const int64_t* offsets, const int64_t* offsets_host, const uint64_t* pos_keys, int64_t nnz,
                             uint32_t* before, int64_t query_block, void* workspace, size_t workspace_bytes, void* stream) {
    return rank_positives(queries, Q, f16_rows(gallery_f16, dim), G, dim, eps, query_labels, gallery_labels, exclude, idx_offset,
                          offsets, offsets_host, pos_keys, nnz, before, query_block, workspace, workspace_bytes,
                          mi355_rank_positives_f16_workspace_bytes(Q, G, dim), stream, "rank_positives_f16");
}

size_t mi355_nearest_centroid_f16_workspace_bytes(int64_t K, int64_t N, int dim) {
    if (K < 1 || N < 1 || dim < 1) return 0;
    return nearest_ws_bytes(K, N, dim, f16_planes_bytes, false);
}

int mi355_nearest_centroid_f16(const float* centroids, int64_t K, const void* rows_f16, int64_t N, int dim, float eps,
                               int64_t query_block, int64_t* assign, float* score, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return nearest_centroid(centroids, K, f16_rows(rows_f16, dim), N, dim, eps, query_block, assign, score, workspace,
                            workspace_bytes, stream, "nearest_centroid_f16");
}

size_t mi355_dbscan_f16_workspace_bytes(int64_t rows, int64_t N, int dim) {
    if (rows < 1 || N < 1 || dim < 1) return 0;
    return dbscan_ws_bytes(rows, N, dim, f16_planes_bytes, false);
}

int mi355_dbscan_degree_f16(const float* queries, int64_t q0, int64_t rows, const void* gallery_f16, int64_t N, int dim, float eps,
                            double threshold, int32_t* degree, void* workspace, size_t workspace_bytes, void* stream) {
    return dbscan_sweep(queries, q0, rows, f16_rows(gallery_f16, dim), N, dim, eps, threshold, 1, degree, nullptr, nullptr, false,
                        workspace, workspace_bytes, stream, "dbscan_degree_f16");
}

int mi355_dbscan_link_f16(const float* queries, int64_t q0, int64_t rows, const void* gallery_f16, int64_t N, int dim, float eps,
                          double threshold, int min_samples, const int32_t* degree, int32_t* parent, uint64_t* border,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return dbscan_sweep(queries, q0, rows, f16_rows(gallery_f16, dim), N, dim, eps, threshold, min_samples,
                        const_cast<int32_t*>(degree), parent, border, true, workspace, workspace_bytes, stream, "dbscan_link_f16");
}

}  // extern "C"
