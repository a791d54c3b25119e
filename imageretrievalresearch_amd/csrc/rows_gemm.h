// Resident rows stored as 128-byte segments (rank_f16.hip: fp16 rows, rank_i8.hip: int8 codes, rank_fp4.hip: packed e2m1
// codes): the one DMA-ring loop of their cosine GEMMs, its family for the tiled launcher and the one driver of their top-k
// searches.  gfx950 only.
#pragma once
#include "rank_common.h"

namespace mi355 {

constexpr int ROWS_KSTEP = 128;               // bytes of a stored row per k-step of the GEMM: one 128-byte segment

// =====================================================================================
// cosine GEMM over resident rows: S / per-tile candidates as k_cos_gemm_split (same block and wave tiling, same launch order,
// same epilogues, rank_common.h).  Block = 4 waves as 2(M) x 2(N), block tile (64 * MT) queries x 128 gallery rows, k-step
// 128 bytes of a row (four 32x32 MFMA sub-steps of 32 bytes, two query planes each).  Everything below is in bytes; ld too.
//   A (query planes, in MFMA-fragment order): 8 * MT pieces of 1 KB per k-step by LDS-DMA from L2, one k-step ahead (ring of 2).
//   B (gallery): the tile's 128 rows x 128 B per k-step by LDS-DMA from HBM, two k-steps ahead (ring of 3).  A piece is 8
//     rows; the 16-byte chunk c of row r lands at position c ^ ((r >> 1) & 7) (applied to the per-lane SOURCE address, the
//     DMA writes lane-linear): row r sits in half (r & 1) of a 256-byte bank row, so the ds_read_b128 of any 16 distinct
//     rows of a lane group hit 16 distinct 16-byte slots.  Rows past G re-read row G - 1 (the epilogue drops them).
// The loop is dma_ring (rank_common.h) with an A ring of 2 and four B pieces per wave: one counted wait and one LDS-only
// barrier per k-step.  Per wave and k-step: 8 * MT + 8 ds_read_b128 and 16 * MT MFMAs.
// LDS: 2 x 32 KB (A) + 3 x 16 KB (B) = 112 KB at MT = 2, 2 x 16 + 48 = 80 KB at MT = 1 (two workgroups per CU).
// A Kind (an object: it may carry pointers) supplies only what the element type changes:
//   Frag, Acc                  a lane's 16 bytes of A or B as the MFMA takes them; its 32x32 accumulator
//   mfma(a, b, c)              c + a . b over one sub-step
//   tail(hi, lo, acc, row0, lane)   the fp32 scores acc[j] of the accumulators hi[j], lo[j] of the hi and lo query planes; they
//                              belong to queries row0 .. row0 + 31
//   ginv()                     what the epilogue multiplies column-wise into the scores, or null
// =====================================================================================
template <class Kind, int MT, class Epi>
__device__ __forceinline__ void rows_gemm_tile(const char* __restrict__ Qs, const char* __restrict__ Gal, const Kind& kind, int Q,
                                               i64 G, int ld, int x0, int ntx, int xtiles, int ny, const Epi& epi) {
    typedef typename Kind::Frag Frag;
    typedef typename Kind::Acc Acc;
    constexpr int BM = 64 * MT;
    constexpr int A_PIECES = (BM / 32) * 8;           // 1 KB pieces per stage: 4 sub-steps x 2 planes per row block
    constexpr int A_STAGE = A_PIECES * 1024;          // bytes per stage
    constexpr int B_STAGE = RK_BN * ROWS_KSTEP;       // bytes per stage (16 KB)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* As = reinterpret_cast<char*>(smem);         // [2][BM/32][4][2][1024]
    char* Bs = As + 2 * A_STAGE;                      // [3][128][128], chunks swizzled

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
    int bx, by;
    rank_tile_of((int)blockIdx.x, xtiles, ny, bx, by);
    const i64 n0 = (i64)(bx + x0) * RK_BN;
    const int m0 = by * BM;
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    const int n_steps = ld / ROWS_KSTEP, n_sub = ld / 32;

    // B: wave w moves pieces 4w .. 4w + 3; lane -> row 8 * piece + lane / 8, LDS position lane % 8
    const char* b_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (swave * 4 + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        const i64 g = n0 + r < G ? n0 + r : G - 1;
        b_src[i] = Gal + g * ld + c * 16;
    }
    // (k-steps past the end re-read the last one: the data is never used, the count of pieces in flight stays uniform)
    auto dma_b = [&](int stage, int t) {
        const int tt = t < n_steps ? t : n_steps - 1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            glds16(reinterpret_cast<const bf16_t*>(b_src[i] + tt * ROWS_KSTEP),
                   reinterpret_cast<bf16_t*>(Bs + stage * B_STAGE + (swave * 4 + i) * 1024));
    };
    // A: piece p = (row block p / 8, sub-step (p % 8) / 2, plane p % 2) of k-step t sits at
    // Qs + ((m0/32 + p/8) * n_sub + 4t) * 2048 + (p % 8) * 1024; wave w moves pieces w, w + 4, ...
    const char* a_src[A_PIECES / 4];
#pragma unroll
    for (int i = 0; i < A_PIECES / 4; ++i) {
        const int p = swave + 4 * i;
        a_src[i] = Qs + ((size_t)(m0 / 32 + p / 8) * n_sub) * 2048 + (p % 8) * 1024 + lane * 16;
    }
    auto dma_a = [&](int buf, int t) {
#pragma unroll
        for (int i = 0; i < A_PIECES / 4; ++i)
            glds16(reinterpret_cast<const bf16_t*>(a_src[i] + (size_t)t * 4 * 2048),
                   reinterpret_cast<bf16_t*>(As + buf * A_STAGE + (swave + 4 * i) * 1024));
    };

    Acc acc_hi[MT][2], acc_lo[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc_hi[i][j][e] = 0; acc_lo[i][j][e] = 0; }

    // B fragment reads: row r = wn * 64 + j * 32 + lr, chunk 2s + (lane >> 5) of sub-step s at its swizzled position
    int b_off[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = wn * 64 + j * 32 + lr;
#pragma unroll
        for (int s = 0; s < 4; ++s) b_off[j][s] = r * ROWS_KSTEP + (((2 * s + (lane >> 5)) ^ ((r >> 1) & 7)) << 4);
    }
    auto compute = [&](int abuf, int bstage) {
        const char* a = As + abuf * A_STAGE + (wm * MT) * 8 * 1024 + lane * 16;
        const char* b = Bs + bstage * B_STAGE;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            Frag bf[2], ah[MT], al[MT];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const Frag*>(b + b_off[j][s]);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                ah[i] = *reinterpret_cast<const Frag*>(a + (i * 8 + s * 2) * 1024);
                al[i] = *reinterpret_cast<const Frag*>(a + (i * 8 + s * 2 + 1) * 1024);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc_lo[i][j] = Kind::mfma(al[i], bf[j], acc_lo[i][j]);
                    acc_hi[i][j] = Kind::mfma(ah[i], bf[j], acc_hi[i][j]);
                }
        }
    };

    dma_ring<2, A_PIECES, 4>(n_steps, swave, dma_a, dma_b, compute);
    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i) kind.tail(acc_hi[i], acc_lo[i], acc[i], m0 + wm * MT * 32 + i * 32, lane);
    epi.tile(acc, smem, kind.ginv(), TileCtx{Q, G, ntx, n0, m0});
}

// The tiled GEMM of a row kind R (launch_tiles, rank_common.h); qry: the queries' planes, gal: the rows, D: their length ld
// in R's own units.  R names its two kernels (the names profiles are keyed by) and passes them their arguments.
template <class R>
struct RowsGemm {
    template <int MT> static constexpr size_t stage_bytes() {   // A ring of 2, B ring of 3
        return (size_t)2 * (64 * MT / 32) * 8 * 1024 + (size_t)3 * RK_BN * ROWS_KSTEP;
    }
    template <int MT, class Epi> static constexpr auto kernel() {
        if constexpr (plain_fk<Epi> >= 0) return R::template plain_kernel<MT, plain_fk<Epi>>();
        else return R::template epi_kernel<MT, Epi>();
    }
    template <int MT, class Epi>
    static void launch(dim3 grid, size_t lds, hipStream_t st, const TileArgs& a, const Epi& epi, int x0, int ntx, int xtiles, int ny) {
        R::launch(kernel<MT, Epi>(), grid, lds, st, a, epi, x0, ntx, xtiles, ny);
    }
};

// mi355_rank_topk_{f16,i8,fp4} and, with filter, their _filtered entries: checks its arguments under the name who.  The row kind R
// supplies ld(dim), planes_bytes, MAX_DIM (0: no cap), SCALED (rows come with scales), gemv(Q, ld) (whether Q queries take
// the GEMV), GEMV_PLANES (its GEMV reads the queries' planes), gemv_launch<NQ>, cos_gemm, its roctx range names and PATH_GEMV.
template <class R>
int rank_topk_rows(const float* queries, int64_t Q, const void* rows, const float* scales, int64_t G, int dim, int k, float eps,
                   int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream,
                   const mi355_rank_filter* filter, const char* who) {
    MI355_REQUIRE(queries && rows && (scales || !R::SCALED) && out_val && out_idx, "%s: null pointer", who);
    MI355_REQUIRE(Q >= 0 && G >= 1 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    if constexpr (R::MAX_DIM > 0) MI355_REQUIRE(dim <= R::MAX_DIM, "%s: dim=%d exceeds %d", who, dim, R::MAX_DIM);
    MI355_REQUIRE(k >= 1 && k <= LARGE_K && k <= G, "%s: k=%d outside [1, %lld]", who, k,
                  (long long)(G < LARGE_K ? G : LARGE_K));
    MI355_REQUIRE(((uintptr_t)rows & 15) == 0, "%s: gallery buffer must be 16-byte aligned", who);
    MI355_REQUIRE(Q <= INT_MAX && G <= ((int64_t)1 << 40), "%s: shape too large Q=%lld G=%lld", who, (long long)Q,
                  (long long)G);
    RankFilter fall{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &fall)) return e;
    if (Q == 0) return OK;
    const int ld = R::ld(dim);
    const bool gemv = R::gemv(Q, ld);    // (Q <= 4: a single query block)
    const RankWs w = carve(workspace, Q, G, dim, k, gemv && !R::GEMV_PLANES ? nullptr : R::planes_bytes, false);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    return search_blocks(
        queries, nullptr, Q, G, dim, k, eps, idx_offset, filter ? &fall : nullptr, out_val, (i64*)out_idx, w, st, "rank/top-k",
        [&](i64 q0, i64 qn, const RankFilter* f) -> int {
            if (gemv) {
                RoctxRange range(R::GEMV_RANGE);
                const unsigned blocks = (unsigned)(cdiv(G, 4) < 4096 ? cdiv(G, 4) : 4096);
                int e;
                switch (qn) {
                    case 1: e = R::template gemv_launch<1>(w, rows, scales, G, dim, ld, blocks, st); break;
                    case 2: e = R::template gemv_launch<2>(w, rows, scales, G, dim, ld, blocks, st); break;
                    case 3: e = R::template gemv_launch<3>(w, rows, scales, G, dim, ld, blocks, st); break;
                    default: e = R::template gemv_launch<4>(w, rows, scales, G, dim, ld, blocks, st);
                }
                if (e) return e;
                MI355_LAUNCH_CHECK();
                set_rank_path(R::PATH_GEMV);
                return OK;
            }
            RoctxRange range(w.cand_val ? R::SELECT_RANGE : R::GEMM_RANGE);
            return with_topk_epi(w, k, f, [&](const auto& epi) {
                return R::cos_gemm(rows, scales, ld, w.qn + q0 * dim, w.qs, qn, G, dim, epi, st);
            });
        });
}

}  // namespace mi355
