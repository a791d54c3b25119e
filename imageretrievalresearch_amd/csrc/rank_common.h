// Shared between the rank kernels (rank.hip: fp32 rows, bf16 planes; rank_f16.hip: fp16 rows; rank_i8.hip: int8 rows): the
// launch order of the cosine GEMM's tiles, its epilogues (one type each: score slab, fused per-tile top-k, ROC histogram, range hits, full-gallery
// ranks, nearest centroid), the host side of the top-k selection that merges what the fused epilogue leaves, the one launcher of every tiled
// GEMM and the query-block loop of every top-k search.  gfx950 only.
#pragma once
#include "common.h"
#include "../../include/mi355_retrieval.h"

#include <limits.h>
#include <math.h>
#include <type_traits>

namespace mi355 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef long long i64;

constexpr float NEG_INF = -INFINITY;
constexpr i64 IDX_PAD = LLONG_MAX;
// Explicit candidate indices (mi355_merge_topk, the unpacked lists of mi355_merge_packed_topk) at or above this are "no
// candidate": IDX_PAD itself and the shard pad 1 << 62.  Such an entry's value is ignored and it never takes a slot; the
// slots that no candidate fills come out as (-inf, IDX_PAD).
constexpr i64 NO_CAND_IDX = (i64)1 << 62;

constexpr int IDX32_PAD = INT_MAX;   // missing candidate in the fused per-tile lists (local int32 indices)

// Order-preserving map float -> uint32 for the fused selection: larger key = better score.  NaN maps to the largest key
// (torch.topk's order), -0 to the key of +0 (they compare equal as floats), every real score to a key > 0.
__device__ __forceinline__ unsigned score_key(float x) {
    const unsigned u = __float_as_uint(x + 0.0f);                  // -0 -> +0
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;       // NaN
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(unsigned key) {
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);   // canonical NaN
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// Ordering of (score, index) candidates: higher score first, ties -> lower index.  NaN orders as the LARGEST value, as in
// torch.topk (a NaN score - e.g. from an Inf/NaN embedding - is returned with its in-range index instead of starving
// the list and leaving pad entries behind); two NaNs tie.
__device__ __forceinline__ bool better(float a, i64 ia, float b, i64 ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return (an && !bn) || (an && bn && ia < ib);
    return (a > b) || (a == b && ia < ib);
}

constexpr int RK_BN = 128;

// Eligibility filter of the filtered searches (mi355_rank_filter): row j of a search with idx_offset is left out for query q
// when exclude[q] == j + idx_offset, or when the label mode rejects gallery_labels[j] against query_labels[q].  qlab / excl
// point at the first query of the call they are handed to (the host shifts them per query block).
struct RankFilter {
    const i64* qlab;      // [Q]; null in MI355_LABEL_ANY
    const i64* glab;      // [G]; null in MI355_LABEL_ANY
    const i64* excl;      // [Q] global row indices (< 0: none), or null
    i64 idx_offset;
    int mode;             // MI355_LABEL_*
};
// The query's side of the filter: its label and the LOCAL row it excludes (-1: none; a row of another shard never matches)
__device__ __forceinline__ void query_filter(const RankFilter& f, i64 q, i64& lab, i64& ex) {
    lab = f.mode != MI355_LABEL_ANY ? f.qlab[q] : 0;
    const i64 e = f.excl ? f.excl[q] : -1;
    ex = e >= 0 ? e - f.idx_offset : -1;
}
__device__ __forceinline__ bool eligible(int mode, i64 qlab, i64 glab, i64 ex, i64 j) {
    const bool lab_ok = mode == MI355_LABEL_ANY || ((glab == qlab) == (mode == MI355_LABEL_SAME));
    return lab_ok && j != ex;
}
constexpr int FILT_LABELS_LD = RK_BN + RK_BN / 32;   // the tile's gallery labels in LDS: one i64 of padding per 32
constexpr size_t FILT_LABELS_BYTES = FILT_LABELS_LD * sizeof(i64);

// 16 bytes per lane from global memory straight into LDS (lane-linear destination; no register is written)
__device__ __forceinline__ void glds16(const bf16_t* gsrc, bf16_t* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// The k loop of every LDS-DMA cosine GEMM (split bf16, prepared planes, fp16 and int8 rows).  dma_a(stage, t) and
// dma_b(stage, t) issue this wave's pieces of k-step t into a ring stage, compute(a stage, b stage) runs a k-step's MFMAs
// out of LDS.  The B ring of 3 runs two k-steps ahead (HBM); the A ring runs one ahead at A_RING = 2 (two buffers, t & 1)
// and two ahead at A_RING = 3, where it shares the B ring's stage numbers.  Every wave issues B_WAVE B pieces per k-step
// (dma_b past the end still issues them, from a harmless source) and A_PIECES / 4 A pieces, plus one if swave <
// A_PIECES % 4.
// No load has a register destination, so the compiler places no vmcnt wait of its own: the one written here is the loop's
// only one.  vmcnt retires in issue order and "vmcnt(N)" waits until at most N of this wave's loads are outstanding, so N
// is the number of pieces issued LAST that may stay in flight.  Step t needs A(t + 1) and B(t + 1) landed at its barrier:
//   A_RING = 2: A(t + 1) is issued in this iteration.  It must come BEFORE B(t + 2) (the two sched_barriers pin that), then
//               N = B_WAVE leaves exactly B(t + 2) in flight and covers A(t + 1) and the older B(t + 1).
//   A_RING = 3: A(t + 2), B(t + 2) are this iteration's; N = B_WAVE + this wave's A pieces leaves both in flight and covers
//               the older A(t + 1), B(t + 1).  With no A(t + 2) left to issue (t + 2 >= n_steps) N = B_WAVE.
// Were the B pieces issued first, N would have to drop to 0 to cover the A pieces and the look-ahead would be lost.
// After lgkmcnt(0) (this wave's LDS reads of step t are done) the barrier publishes step t + 1 and frees step t's stages
// for the next iteration's DMA.  The closing __syncthreads() drains the last look-ahead pieces before smem is reused.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int A_RING, int A_PIECES, int B_WAVE, class DmaA, class DmaB, class Compute>
__device__ __forceinline__ void dma_ring(int n_steps, int swave, const DmaA& dma_a, const DmaB& dma_b, const Compute& compute) {
    static_assert(A_RING == 2 || A_RING == 3, "the A ring is one or two k-steps ahead");
    dma_a(0, 0);
    if (A_RING == 3 && n_steps > 1) dma_a(1, 1);
    dma_b(0, 0);
    dma_b(1, 1);
    __syncthreads();                   // drains vmcnt: everything has landed

    int bs_cur = 0, bs_far = 2;        // ring stage of k-step t / of k-step t + 2
    for (int t = 0; t < n_steps; ++t) {
        if constexpr (A_RING == 2) {
            if (t + 1 < n_steps) dma_a((t & 1) ^ 1, t + 1);  // everybody left this buffer at the previous barrier
        } else {
            if (t + 2 < n_steps) dma_a(bs_far, t + 2);
        }
        __builtin_amdgcn_sched_barrier(0);
        dma_b(bs_far, t + 2);
        __builtin_amdgcn_sched_barrier(0);
        compute(A_RING == 2 ? (t & 1) : bs_cur, bs_cur);
        if (A_RING == 2 || t + 2 >= n_steps) wait_vmcnt<B_WAVE>();
        else if (swave < A_PIECES % 4) wait_vmcnt<B_WAVE + A_PIECES / 4 + 1>();
        else wait_vmcnt<B_WAVE + A_PIECES / 4>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        bs_cur = bs_cur == 2 ? 0 : bs_cur + 1;
        bs_far = bs_far == 2 ? 0 : bs_far + 1;
    }
    __syncthreads();
}

// Launch order of the GEMM tiles (speed only, every result is the same for any order): the grid is one-dimensional and the
// query blocks of ONE gallery tile get the linear ids L, L + 8, L + 16, ...  The dispatcher deals workgroups round-robin
// over the 8 XCDs, so those workgroups share an L2 and start in the same round: the gallery tile comes from HBM once and
// the other query blocks hit it in L2.  (With a (tile, query block) grid, x fastest, all tiles of query block 0 filled the
// machine before query block 1 started: PMC showed every gallery row fetched from HBM once per query block.)
__device__ __forceinline__ void rank_tile_of(int L, int ntiles, int ny, int& tx, int& ty) {
    const int full = (ntiles >> 3) << 3;
    if (L < full * ny) {
        const int g = L / (8 * ny), r = L - g * 8 * ny;
        tx = g * 8 + (r & 7);
        ty = r >> 3;
    } else {
        const int r = L - full * ny, rem = ntiles - full;
        ty = r / rem;
        tx = full + r - ty * rem;
    }
}

// ---- the epilogues of the tiled cosine GEMM.  Every loop (exact fp32, split bf16, prepared planes, fp16 rows) leaves the same
// accumulator layout (the C/D map of the 32x32 MFMAs does not depend on the input type) and ends in epi.tile(acc, smem, ginv,
// t), after a __syncthreads() that retired every read of its staging buffers (smem is reused).  An epilogue is one type:
//   its arguments (the members; it travels to the kernel by value),
//   tile(): what a workgroup does with its (64 * MT) x 128 accumulators; scores are acc * ginv[col] in every epilogue,
//   lds_bytes<STAGE>(): the dynamic LDS of a kernel whose loop stages STAGE bytes.
// Where a workgroup's tile lies: queries [m0, m0 + 64 * MT) of Q, gallery rows [n0, n0 + 128) of G (ntx column tiles)
struct TileCtx {
    int Q;
    i64 G;
    int ntx;
    i64 n0;
    int m0;
};

// ---- adjusted scores (mi355_rank_topk_adjusted, mi355_cosine_scores_adjusted; CSLS and cohort normalisation, scorenorm.hip):
// the score s of pair (query q, gallery row g) becomes t = s * (aq[q] + ag[g]) - (bq[q] + bg[g]), every step rounded to fp32
// and none fused, so t depends on s and the four coefficients alone.  A null vector counts as 0.  aq / bq point at the first
// query of the call they are handed to (the host shifts them per query block, as it shifts the filter).
struct NoAdjust {};
struct ScoreAdjust {
    const float* aq;            // [Q] or null
    const float* bq;            // [Q] or null
    const float* ag;            // [G] or null
    const float* bg;            // [G] or null
};
__device__ __forceinline__ float adjusted_score(float s, float w, float c) {
    float p = __fmul_rn(s, w);
    asm volatile("" : "+v"(p));     // the rounded product in a register: -ffp-contract=fast must not fuse it into the subtraction
    return __fsub_rn(p, c);
}
// aq or bq of a lane's query row in the MFMA layout: one accumulator element belongs to row urow in lanes 0-31 and to row
// urow + 4 in lanes 32-63, urow the same in the whole wave.  Both rows are read through wave-uniform addresses, so the loads are
// scalar and no vector register holds a coefficient across the tile (as vector loads, hoisted in front of the tile's stores,
// they cost the 128-query kernels up to 34 VGPRs and with them a wave per SIMD); the lane then picks its own.  Rows past Q: 0.
__device__ __forceinline__ float row_coefficient(const float* v, int urow, int Q, int upper) {
    const float lo = (v && urow < Q) ? v[urow] : 0.0f;
    const float hi = (v && urow + 4 < Q) ? v[urow + 4] : 0.0f;
    return upper ? hi : lo;
}
// The block of queries [q0, ...) of a
inline ScoreAdjust adjust_from(const ScoreAdjust& a, i64 q0) {
    ScoreAdjust r = a;
    if (r.aq) r.aq += q0;
    if (r.bq) r.bq += q0;
    return r;
}

// The score slab S [Q][G]
struct SlabEpi {
    float* S;
    template <size_t STAGE> static constexpr size_t lds_bytes() { return STAGE; }
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float*, const float* __restrict__ ginv, const TileCtx& t) const {
        const int Q = t.Q, m0 = t.m0;
        const i64 G = t.G, n0 = t.n0;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
        // C[row = query][col = gallery]; lane: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const i64 col = n0 + wn * 64 + j * 32 + lr;
            if (col >= G) continue;
            const float gs = ginv ? ginv[col] : 1.0f;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (row < Q) S[(i64)row * G + col] = acc[i][j][r] * gs;
                }
            }
        }
    }
};

// The adjusted score slab T [Q][G]: SlabEpi with the map applied.  The gallery side's coefficients are read once per lane
// column, the query side's once per row (32 lanes share the address; an L2 hit after the first tile).
struct AdjSlabEpi {
    float* S;
    ScoreAdjust adj;
    template <size_t STAGE> static constexpr size_t lds_bytes() { return STAGE; }
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float*, const float* __restrict__ ginv, const TileCtx& t) const {
        const int Q = t.Q, m0 = t.m0;
        const i64 G = t.G, n0 = t.n0;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
        float gs[2], ga[2], gb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const i64 col = n0 + wn * 64 + j * 32 + lr;
            gs[j] = (ginv && col < G) ? ginv[col] : 1.0f;
            ga[j] = (adj.ag && col < G) ? adj.ag[col] : 0.0f;
            gb[j] = (adj.bg && col < G) ? adj.bg[col] : 0.0f;
        }
        // C[row = query][col = gallery]; lane: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
        const int urow0 = m0 + __builtin_amdgcn_readfirstlane(wm) * MT * 32;     // wave-uniform
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int urow = urow0 + i * 32 + (r & 3) + 8 * (r >> 2), row = urow + 4 * (lane >> 5);
                const float qa = row_coefficient(adj.aq, urow, Q, lane >> 5), qb = row_coefficient(adj.bq, urow, Q, lane >> 5);
                if (row >= Q) continue;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const i64 col = n0 + wn * 64 + j * 32 + lr;
                    if (col < G) S[(i64)row * G + col] = adjusted_score(acc[i][j][r] * gs[j], qa + ga[j], qb + gb[j]);
                }
            }
        }
    }
};

constexpr size_t EPI_TILE_BYTES = (size_t)64 * (RK_BN + 4) * sizeof(float);   // the fused selection's transposed score tile

// The fused selection (k <= FK): the score tile never leaves the CU, k (score, local int32 index) candidates per (query,
// column tile) go to cand_val / cand_idx [Q][ntx][k].
// FILT: columns the filter rejects enter the selection as key 0, i.e. never.  The tile's 128 gallery labels are read once per
// workgroup into LDS behind the transposed tile (64 x 132 floats + 1 KB stays inside every loop's staging buffers, so the
// LDS request and the resident workgroups per CU are those of the unfiltered kernel).
// Adj = ScoreAdjust (mi355_rank_topk_adjusted): the tile is written as adjusted scores and the same selection runs on it; the
// map needs no LDS of its own.  Adj = NoAdjust takes no room in the object and compiles to the unadjusted selection.
// The two epilogue types are SelectEpi<FK, FILT> and AdjSelectEpi<FK, FILT> below (kernel names are made of the type's name).
template <int FK, bool FILT, class Adj>
struct SelectTile {
    int k;
    float* cand_val;
    int* cand_idx;
    RankFilter flt;             // FILT: the filter of this call's queries
    [[no_unique_address]] Adj adj;
    // LDS: the staging buffers, or the transposed score tile (64 rows at a time) if that is larger
    template <size_t STAGE> static constexpr size_t lds_bytes() {
        static_assert(!FILT || STAGE >= EPI_TILE_BYTES + FILT_LABELS_BYTES, "the filtered epilogue would grow the GEMM's LDS");
        return EPI_TILE_BYTES > STAGE ? EPI_TILE_BYTES : STAGE;
    }
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const {
        static_assert(FK > 0, "the fused selection keeps at least one candidate");
        const int Q = t.Q, ntx = t.ntx, m0 = t.m0;
        const i64 G = t.G, n0 = t.n0;
        constexpr int BM = 64 * MT;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
        // (the loop's last __syncthreads() retired every read of the staging buffers)
        // 64 query rows at a time, so that the transposed tile (64 x 132 floats = 33.8 KB) fits inside the staging
        // buffers: a bigger LDS request would cost the third resident workgroup per CU and with it a round of tiles
        constexpr int CLD = RK_BN + 4;                 // 132 floats: a thread per row reads float4s conflict-free
        float* Ct = smem;                              // [64][CLD]
        const i64 ncol = (G - n0 < RK_BN) ? G - n0 : RK_BN;     // valid columns of this tile
        i64* glab = reinterpret_cast<i64*>(smem + 64 * CLD);    // FILT: [4][33], label of column c at c + c / 32
        if constexpr (FILT) {
            if (tid < RK_BN) glab[tid + (tid >> 5)] = (flt.mode != MI355_LABEL_ANY && tid < ncol) ? flt.glab[n0 + tid] : 0;
        }
#pragma unroll 1
        for (int h = 0; h < BM / 64; ++h) {
            if ((wm * MT * 32) / 64 == h) {            // this wave's rows belong to pass h
                if constexpr (std::is_same_v<Adj, NoAdjust>) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const i64 col = n0 + wn * 64 + j * 32 + lr;
                        const float gs = (ginv && col < G) ? ginv[col] : 1.0f;
#pragma unroll
                        for (int i = 0; i < MT; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int row = (wm * MT * 32) % 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                                Ct[row * CLD + wn * 64 + j * 32 + lr] = acc[i][j][r] * gs;
                            }
                    }
                } else {
                    // the gallery side's coefficients once per lane column, the query side's once per row (rows past Q: 0)
                    float gs[2], ga[2], gb[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const i64 col = n0 + wn * 64 + j * 32 + lr;
                        gs[j] = (ginv && col < G) ? ginv[col] : 1.0f;
                        ga[j] = (adj.ag && col < G) ? adj.ag[col] : 0.0f;
                        gb[j] = (adj.bg && col < G) ? adj.bg[col] : 0.0f;
                    }
                    const int urow0 = m0 + h * 64 + (__builtin_amdgcn_readfirstlane(wm) * MT * 32) % 64;     // wave-uniform
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = (wm * MT * 32) % 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                            const int urow = urow0 + i * 32 + (r & 3) + 8 * (r >> 2);
                            const float qa = row_coefficient(adj.aq, urow, Q, lane >> 5);
                            const float qb = row_coefficient(adj.bq, urow, Q, lane >> 5);
#pragma unroll
                            for (int j = 0; j < 2; ++j)
                                Ct[row * CLD + wn * 64 + j * 32 + lr] = adjusted_score(acc[i][j][r] * gs[j], qa + ga[j], qb + gb[j]);
                        }
                }
            }
            __syncthreads();
            // Selection: FOUR threads per query row, each scans 32 columns in ascending order into a sorted FK-list held as
            // order-preserving integer keys (NaN = largest, -0 = +0); the insertion is branch-free (a divergent insertion
            // sort cost 10 % of the tile: some lane of the wave inserts at almost every column) and skipped by a wave vote
            // when no lane beats its FK-th entry.  The row's four lists are merged through shuffles in column order, so
            // ties keep resolving to the lower index.
            {
                const int lrow = tid >> 2, part = tid & 3;
                unsigned kv[FK];
                int ki[FK];
#pragma unroll
                for (int i = 0; i < FK; ++i) { kv[i] = 0u; ki[i] = IDX32_PAD; }      // key 0 = below every real score (-inf is 0x007fffff)
                auto insert = [&](unsigned key, int id) {
                    bool g[FK];
#pragma unroll
                    for (int i = 0; i < FK; ++i) g[i] = key > kv[i];          // strict: an equal score keeps the earlier (lower) index
#pragma unroll
                    for (int i = FK - 1; i > 0; --i) {
                        kv[i] = g[i] ? (g[i - 1] ? kv[i - 1] : key) : kv[i];
                        ki[i] = g[i] ? (g[i - 1] ? ki[i - 1] : id) : ki[i];
                    }
                    kv[0] = g[0] ? key : kv[0];
                    ki[0] = g[0] ? id : ki[0];
                };
                const float* rowp = Ct + lrow * CLD + part * 32;
                i64 fq_lab = 0, fq_ex = -1;
                if constexpr (FILT) {
                    if (m0 + h * 64 + lrow < Q) query_filter(flt, m0 + h * 64 + lrow, fq_lab, fq_ex);
                }
#pragma unroll 2
                for (int c4i = 0; c4i < 8; ++c4i) {
                    const f32x4 v4 = *reinterpret_cast<const f32x4*>(rowp + c4i * 4);
                    const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = part * 32 + c4i * 4 + e;
                        unsigned key = score_key(vv[e]);
                        if (c >= ncol) key = 0u;
                        if constexpr (FILT) {
                            if (!eligible(flt.mode, fq_lab, glab[c + part], fq_ex, n0 + c)) key = 0u;
                        }
                        if (__any(key > kv[FK - 1])) insert(key, (int)n0 + c);      // n0 + c < 2^31 (checked on the host)
                    }
                }
                // merge parts 1..3 into part 0 (lanes 4r .. 4r+3 of one wave)
#pragma unroll
                for (int src = 1; src < 4; ++src) {
#pragma unroll
                    for (int i = 0; i < FK; ++i) {
                        const unsigned ok = (unsigned)__shfl(kv[i], (lane & ~3) + src, 64);
                        const int oi = __shfl(ki[i], (lane & ~3) + src, 64);
                        if (part == 0) insert(ok, oi);
                    }
                }
                const int qrow = m0 + h * 64 + lrow;
                if (part == 0 && qrow < Q) {
                    const size_t o = ((size_t)qrow * ntx + (size_t)(n0 / RK_BN)) * k;
#pragma unroll
                    for (int i = 0; i < FK; ++i)
                        if (i < k) { cand_val[o + i] = ki[i] == IDX32_PAD ? NEG_INF : key_score(kv[i]); cand_idx[o + i] = ki[i]; }
                }
            }
            __syncthreads();
        }
    }
};
template <int FK, bool FILT> struct SelectEpi : SelectTile<FK, FILT, NoAdjust> {};
template <int FK, bool FILT> struct AdjSelectEpi : SelectTile<FK, FILT, ScoreAdjust> {};

// ---- verification ROC (mi355_roc_pairs_hist[_f16]): the histogram epilogue bins every (query, gallery row) score of the
// tile by (genuine / impostor, threshold) into a per-workgroup histogram; the score slab never exists.
// Bin b of a score s = the number of thresholds t with s >= t (0 .. T), compared in fp32 against the fp32 CEILING of each
// float64 t (the smallest float f with (double)f >= t), which is exactly the float64 comparison for every fp32 score.
// A NaN score lands in bin 0 (below every threshold).
constexpr int ROC_MAX_T = MI355_ROC_MAX_THRESHOLDS;
constexpr int ROC_SUB_T = 1024;                         // T <= this: one sub-histogram per wave (less LDS-atomic contention)
constexpr int ROC_BIN_WORDS = ROC_MAX_T + 4;            // = 4 * (ROC_SUB_T + 1): either layout fits
// LDS of the histogram epilogue: threshold table, bins, the tile's gallery labels, its query labels and excluded rows
constexpr size_t ROC_EPI_BYTES = (size_t)ROC_MAX_T * sizeof(float) + (size_t)ROC_BIN_WORDS * sizeof(unsigned) +
                                 (size_t)3 * RK_BN * sizeof(i64);

__host__ __device__ __forceinline__ float roc_ceil_f32(double t) {
    float f = (float)t;                                 // round to nearest
    if ((double)f < t) f = nextafterf(f, INFINITY);
    return f;
}

struct RocArgs {
    const i64* qlab;            // [Q] labels of the queries of this call (the host shifts them per query block)
    const i64* glab;            // [G] labels of the gallery rows
    const i64* excl;            // [Q] global row indices (< 0: none), or null: pair (q, j) is not counted if excl[q] == j + idx_offset
    i64 idx_offset;
    const double* thr;          // [T] the thresholds, ascending, finite
    unsigned long long* hist;   // [2][T + 1]: genuine / impostor pairs per bin (accumulated)
    int T;
    int top;                    // largest power of two <= T (binary search)
    int uniform;                // 1: guess the bin as 1 + (s - ceil(thr[0])) * scale, then fix it with compares
    float scale;
    template <size_t STAGE> static constexpr size_t lds_bytes() { return ROC_EPI_BYTES > STAGE ? ROC_EPI_BYTES : STAGE; }
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const;
};

// The bin of score s against the ascending table tab[T] in LDS (fp32 ceilings; float64 thresholds for float64 scores)
template <class V>
__device__ __forceinline__ int roc_bin(V s, const V* tab, const RocArgs& a) {
    if (a.uniform) {
        if (!(s >= tab[0])) return 0;                   // NaN or below the grid
        const V x = (s - tab[0]) * (V)a.scale;
        int g = x < (V)(a.T - 1) ? (int)x + 1 : a.T;
        while (g < a.T && s >= tab[g]) ++g;             // (a uniform grid: at most a step or two either way)
        while (s < tab[g - 1]) --g;
        return g;
    }
    int b = 0;                                          // count of tab[] <= s; NaN compares false
    for (int step = a.top; step > 0; step >>= 1)
        if (b + step <= a.T && tab[b + step - 1] <= s) b += step;
    return b;
}

// The histogram epilogue.  Scores are acc * ginv[col] as in the other epilogues, so every pair gets the bits of
// mi355_cosine_scores on the same loop.  Counts go into LDS as ONE u32 per bin holding both classes (genuine adds 1 << 16,
// impostor 1: a tile has at most 128 x 128 = 16384 pairs, the halves cannot carry), then to roc.hist with one 64-bit atomic
// per non-zero (bin, class), one lane per bin.
template <int MT>
__device__ __forceinline__ void RocArgs::tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const {
    const RocArgs& roc = *this;
    const int Q = t.Q, m0 = t.m0;
    const i64 G = t.G, n0 = t.n0;
    constexpr int BM = 64 * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
    const int T = roc.T, nb = T + 1;
    const bool sub = T <= ROC_SUB_T;
    float* tab = smem;                                                       // [T]
    unsigned* bins = reinterpret_cast<unsigned*>(smem + ROC_MAX_T);          // [sub ? 4 : 1][T + 1]
    i64* glab = reinterpret_cast<i64*>(bins + ROC_BIN_WORDS);                // [128]
    i64* qlab = glab + RK_BN;                                                // [BM]
    i64* qex = qlab + RK_BN;                                                 // [BM] LOCAL excluded row, -1: none
    for (int i = tid; i < T; i += 256) tab[i] = roc_ceil_f32(roc.thr[i]);
    for (int i = tid; i < (sub ? 4 * nb : nb); i += 256) bins[i] = 0u;
    if (tid < RK_BN) glab[tid] = n0 + tid < G ? roc.glab[n0 + tid] : 0;
    if (tid < BM) {
        const bool ok = m0 + tid < Q;
        const i64 e = ok && roc.excl ? roc.excl[m0 + tid] : -1;
        qlab[tid] = ok ? roc.qlab[m0 + tid] : 0;
        qex[tid] = e >= 0 ? e - roc.idx_offset : -1;
    }
    __syncthreads();
    unsigned* mine = bins + (sub ? wave * nb : 0);
    // C[row = query][col = gallery]; lane: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = wn * 64 + j * 32 + lr;
        const i64 col = n0 + c;
        if (col < G) {
            const float gs = ginv ? ginv[col] : 1.0f;
            const i64 gl = glab[c];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m0 + row < Q && col != qex[row])
                        atomicAdd(&mine[roc_bin(acc[i][j][r] * gs, tab, roc)], qlab[row] == gl ? 0x10000u : 1u);
                }
        }
    }
    __syncthreads();
    for (int b = tid; b < nb; b += 256) {
        unsigned u = bins[b];
        if (sub) u += bins[nb + b] + bins[2 * nb + b] + bins[3 * nb + b];
        if (u >> 16) atomicAdd(&roc.hist[b], (unsigned long long)(u >> 16));
        if (u & 0xffffu) atomicAdd(&roc.hist[nb + b], (unsigned long long)(u & 0xffffu));
    }
}

// ---- cosine range search (mi355_cosine_range[_f16]): the range epilogue keeps every (query, gallery row) pair whose score
// is >= the threshold (float64 comparison: fp32 score >= roc_ceil_f32(t); NaN never), filtered as the top-k search filters.
// Per (query row, column tile) the hits are a bit mask in LDS; one 64-bit atomic per workgroup reserves the tile's hits in a
// candidate buffer, where each row's hits land in ascending column order, and (start, count) of each (query, tile) goes to
// a table that the compaction (range.hip) walks in tile order: the output never depends on the order of the atomics.
// LDS of the range epilogue: hit masks [BM][4] u32, row counts / prefixes [BM], the workgroup's base, then the tile's gallery
// labels [128], its query labels and LOCAL excluded rows [BM]
constexpr size_t RANGE_EPI_BYTES = (size_t)128 * 4 * sizeof(unsigned) + (size_t)128 * sizeof(int) + 2 * sizeof(i64) +
                                   (size_t)(RK_BN + 2 * 128) * sizeof(i64);

struct RangeArgs {
    RankFilter f;               // the filter of this call's queries (mode ANY and excl null: none)
    float thr;                  // roc_ceil_f32(threshold)
    unsigned long long* cursor; // hits of this GEMM call so far (zeroed by the host before it)
    unsigned long long* raw;    // [cap] hits {local column | score bits << 32}, chunks in reservation order
    i64 cap;                    // entries raw holds: a tile whose chunk would pass it writes nothing (the counts stay exact)
    i64* tstart;                // [Q][ntx] first raw entry of (query, column tile)
    int* tcount;                // [Q][ntx] its hits
    int keep_all;               // 1: every eligible pair is a hit whatever its score, NaN included (mi355_positives_range)
    template <size_t STAGE> static constexpr size_t lds_bytes() {   // inside the staging buffers of every loop
        static_assert(STAGE >= RANGE_EPI_BYTES, "the range epilogue would grow the GEMM's LDS");
        return STAGE;
    }
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const;
};

// The range epilogue.  Scores are acc * ginv[col] as in the other epilogues: every hit has the bits of mi355_cosine_scores on
// the same loop.
template <int MT>
__device__ __forceinline__ void RangeArgs::tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const {
    const RangeArgs& rg = *this;
    const int Q = t.Q, ntx = t.ntx, m0 = t.m0;
    const i64 G = t.G, n0 = t.n0;
    constexpr int BM = 64 * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
    unsigned* mask = reinterpret_cast<unsigned*>(smem);                      // [BM][4]: bit c % 32 of word c / 32 = column c
    int* rpre = reinterpret_cast<int*>(mask + 128 * 4);                      // [BM] hits of row, then their exclusive prefix
    unsigned long long* sbase = reinterpret_cast<unsigned long long*>(rpre + 128);   // [0] the reservation, [1] the total
    i64* glab = reinterpret_cast<i64*>(sbase + 2);                           // [128]
    i64* qlab = glab + RK_BN;                                                // [BM]
    i64* qex = qlab + 128;                                                   // [BM] LOCAL excluded row, -1: none
    const bool filt = rg.f.mode != MI355_LABEL_ANY || rg.f.excl;
    if (filt) {
        if (tid < RK_BN) glab[tid] = rg.f.mode != MI355_LABEL_ANY && n0 + tid < G ? rg.f.glab[n0 + tid] : 0;
        if (tid < BM) {
            i64 l = 0, e = -1;
            if (m0 + tid < Q) query_filter(rg.f, m0 + tid, l, e);
            qlab[tid] = l;
            qex[tid] = e;
        }
        __syncthreads();
    }
    // 1. the hit masks: in the MFMA layout lanes 0-31 hold 32 consecutive columns of one row, lanes 32-63 those of row + 4,
    //    so one ballot is two whole mask words; each (row, word) belongs to exactly one wave
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = wn * 64 + j * 32 + lr;
        const i64 col = n0 + c;
        const float gs = (ginv && col < G) ? ginv[col] : 1.0f;
        const i64 gl = filt ? glab[c] : 0;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                bool hit = col < G && m0 + row < Q && (rg.keep_all || acc[i][j][r] * gs >= rg.thr);
                if (filt) hit = hit && eligible(rg.f.mode, qlab[row], gl, qex[row], col);
                const unsigned long long b = __ballot(hit);
                if (lane == 0) {
                    mask[row * 4 + wn * 2 + j] = (unsigned)b;
                    mask[(row + 4) * 4 + wn * 2 + j] = (unsigned)(b >> 32);
                }
            }
    }
    __syncthreads();
    // 2. per row: its hits, their exclusive prefix over the tile's rows (a scan per wave, waves 0 and 1), ONE reservation
    int cnt = 0, incl = 0;
    if (tid < BM) {
        cnt = __popc(mask[tid * 4]) + __popc(mask[tid * 4 + 1]) + __popc(mask[tid * 4 + 2]) + __popc(mask[tid * 4 + 3]);
        incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (tid == 63) sbase[1] = (unsigned long long)incl;                  // wave 0's total
    }
    __syncthreads();
    if (tid < BM) {
        if (tid >= 64) incl += (int)sbase[1];
        rpre[tid] = incl - cnt;
        if (tid == BM - 1) sbase[0] = incl > 0 ? atomicAdd(rg.cursor, (unsigned long long)incl) : 0ull;
    }
    __syncthreads();
    const unsigned long long base = sbase[0];
    const int tile = (int)(n0 / RK_BN);
    if (tid < BM && m0 + tid < Q) {
        const size_t t = (size_t)(m0 + tid) * ntx + tile;
        rg.tstart[t] = (i64)base + rpre[tid];
        rg.tcount[t] = cnt;
    }
    const int total = rpre[BM - 1] + __popc(mask[(BM - 1) * 4]) + __popc(mask[(BM - 1) * 4 + 1]) + __popc(mask[(BM - 1) * 4 + 2]) +
                      __popc(mask[(BM - 1) * 4 + 3]);
    if (total == 0 || (i64)base + total > rg.cap) return;                   // nothing to write, or past the buffer: counts only
    // 3. every hit from its accumulator to base + row prefix + the popcount of the row's bits before it
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = wn * 64 + j * 32 + lr, w = wn * 2 + j;
        const i64 col = n0 + c;
        const float gs = (ginv && col < G) ? ginv[col] : 1.0f;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const unsigned* m = mask + row * 4;
                if ((m[w] >> lr) & 1u) {
                    int before = __popc(m[w] & ((1u << lr) - 1u));
                    for (int u = 0; u < w; ++u) before += __popc(m[u]);
                    const float s = acc[i][j][r] * gs;
                    rg.raw[base + rpre[row] + before] = (unsigned long long)(unsigned)col |
                                                        ((unsigned long long)__float_as_uint(s) << 32);
                }
            }
    }
}

// ---- full-gallery ranks (mi355_rank_positives[_f16]): the ranks epilogue counts, per query, every eligible row that is
// NOT a positive (label differs) into one bin: the number b of the query's positives that rank before it.  The order is the
// top-k search's, as one 64-bit composite per (score, row): higher score_key first, on equal keys the lower row.  The query's
// positives are given as their composites in descending order (keys, CSR over the queries); bin b = R_q (the row beats no
// positive) is never needed and never written.  Counts are integers: the result does not depend on the order of the atomics.
__host__ __device__ __forceinline__ unsigned long long rank_composite(unsigned key, unsigned local_row) {
    return ((unsigned long long)key << 32) | (unsigned)~local_row;
}

// LDS of the ranks epilogue: the tile's gallery labels [128], its query labels, LOCAL excluded rows and CSR starts [BM] (i64),
// each query's weakest positive composite [BM] and its R_q [BM]
constexpr size_t RANKS_EPI_BYTES = (size_t)(RK_BN + 3 * 128) * sizeof(i64) + (size_t)128 * sizeof(unsigned long long) +
                                   (size_t)128 * sizeof(int);

struct RanksArgs {
    const i64* qlab;            // [Q] labels of the queries of this call (the host shifts them per query block)
    const i64* glab;            // [G] labels of the gallery rows
    const i64* excl;            // [Q] global row indices (< 0: none), or null
    i64 idx_offset;
    const i64* offsets;         // [Q + 1] of this call's queries: positions in keys / before (absolute, not per block)
    const unsigned long long* keys;   // [nnz] composites of each query's positives, descending
    unsigned* before;           // [nnz] before[offsets[q] + b] += 1 per negative that exactly b positives of q beat
    template <size_t STAGE> static constexpr size_t lds_bytes() {   // inside the staging buffers of every loop
        static_assert(STAGE >= RANKS_EPI_BYTES, "the ranks epilogue would grow the GEMM's LDS");
        return STAGE;
    }
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const;
};

// The ranks epilogue.  Scores are acc * ginv[col] as in the other epilogues: every negative is compared with the bits of
// mi355_cosine_scores on the same loop, the bits the positives' composites were made from.  For a trained model most
// negatives lose against the query's weakest positive and are done after one 64-bit compare; the others binary-search the
// query's composites in global memory (an L2-resident segment) and add one to their bin.
template <int MT>
__device__ __forceinline__ void RanksArgs::tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const {
    const RanksArgs& rk = *this;
    const int Q = t.Q, m0 = t.m0;
    const i64 G = t.G, n0 = t.n0;
    constexpr int BM = 64 * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
    i64* glab = reinterpret_cast<i64*>(smem);                                // [128]
    i64* qlab = glab + RK_BN;                                                // [BM]
    i64* qex = qlab + 128;                                                   // [BM] LOCAL excluded row, -1: none
    i64* qstart = qex + 128;                                                 // [BM] first position of the query's segment
    unsigned long long* qweak = reinterpret_cast<unsigned long long*>(qstart + 128);   // [BM] its last (weakest) composite
    int* qR = reinterpret_cast<int*>(qweak + 128);                           // [BM] its length R_q (< 2^31: G is)
    if (tid < RK_BN) glab[tid] = n0 + tid < G ? rk.glab[n0 + tid] : 0;
    if (tid < BM) {
        const bool ok = m0 + tid < Q;
        const i64 e = ok && rk.excl ? rk.excl[m0 + tid] : -1;
        const i64 s0 = ok ? rk.offsets[m0 + tid] : 0, s1 = ok ? rk.offsets[m0 + tid + 1] : 0;
        qlab[tid] = ok ? rk.qlab[m0 + tid] : 0;
        qex[tid] = e >= 0 ? e - rk.idx_offset : -1;
        qstart[tid] = s0;
        qR[tid] = (int)(s1 - s0);
        qweak[tid] = s1 > s0 ? rk.keys[s1 - 1] : 0ull;
    }
    __syncthreads();
    // C[row = query][col = gallery]; lane: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = wn * 64 + j * 32 + lr;
        const i64 col = n0 + c;
        if (col < G) {
            const float gs = ginv ? ginv[col] : 1.0f;
            const i64 gl = glab[c];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m0 + row >= Q || col == qex[row] || qlab[row] == gl) continue;      // not eligible, or a positive
                    const int R = qR[row];
                    const unsigned long long K = rank_composite(score_key(acc[i][j][r] * gs), (unsigned)col);
                    if (R == 0 || K < qweak[row]) continue;                  // beats no positive: bin R_q, never needed
                    // b = the positives that beat K = the first position whose composite is below K (the last one is)
                    const unsigned long long* seg = rk.keys + qstart[row];
                    int lo = 0, hi = R - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (seg[mid] > K) lo = mid + 1; else hi = mid;
                    }
                    atomicAdd(&rk.before[qstart[row] + lo], 1u);
                }
        }
    }
}

// ---- nearest centroid (mi355_nearest_centroid[_f16]): the centroids are the GEMM's query rows, the resident rows its gallery
// columns, and the nearest epilogue keeps per COLUMN the best (score, centroid) over the tile's query rows - the arg-max runs
// down the rows, the opposite direction to SelectEpi.  "Best" is the maximum of one 64-bit key, score_key in the high word
// and ~centroid in the low one: the higher score wins, equal scores go to the lower centroid.  A maximum does not depend on
// the order it is taken in, so best[] has the same bits for any launch order and any split of the centroids into GEMM calls.
__host__ __device__ __forceinline__ unsigned long long nearest_key(unsigned key, unsigned centroid) {
    return ((unsigned long long)key << 32) | (unsigned)~centroid;
}

struct NearestEpi {
    unsigned long long* best;   // [G] keys, zeroed by the host before the first GEMM call (every real score's key is > 0)
    int q0;                     // centroid index of this call's first query row
    template <size_t STAGE> static constexpr size_t lds_bytes() {   // 128 keys: inside the staging buffers of every loop
        static_assert(STAGE >= RK_BN * sizeof(unsigned long long), "the nearest epilogue would grow the GEMM's LDS");
        return STAGE;
    }
    // Scores are acc * ginv[col] as in the other epilogues: the bits of mi355_cosine_scores on the same loop.
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const {
        const int Q = t.Q, m0 = t.m0;
        const i64 G = t.G, n0 = t.n0;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
        unsigned long long* colbest = reinterpret_cast<unsigned long long*>(smem);   // [128]: the upper row half's keys
        unsigned long long mine[2];
        // C[row = query][col = gallery]; lane: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const i64 col = n0 + wn * 64 + j * 32 + lr;
            const float gs = (ginv && col < G) ? ginv[col] : 1.0f;
            // 1. in registers over the lane's 16 * MT rows, ascending: a strict compare keeps the lower centroid
            unsigned bk = 0u;
            int brow = 0;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const unsigned key = row < Q ? score_key(acc[i][j][r] * gs) : 0u;
                    if (key > bk) { bk = key; brow = row; }
                }
            unsigned long long k64 = bk ? nearest_key(bk, (unsigned)(q0 + brow)) : 0ull;
            // 2. the partner lane holds the column's other rows (row + 4 of every group of 8)
            const unsigned long long o = __shfl_xor(k64, 32, 64);
            mine[j] = o > k64 ? o : k64;
        }
        // 3. the two row halves of the tile (wm) through LDS, then ONE global maximum per column per workgroup
        if (wm == 1 && lane < 32) {
            colbest[wn * 64 + lr] = mine[0];
            colbest[wn * 64 + 32 + lr] = mine[1];
        }
        __syncthreads();
        if (wm == 0 && lane < 32) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = wn * 64 + j * 32 + lr;
                const unsigned long long o = colbest[c], k64 = o > mine[j] ? o : mine[j];
                if (n0 + c < G && k64) atomicMax(&best[n0 + c], k64);
            }
        }
    }
};

// ---- DBSCAN / threshold components (mi355_dbscan_degree[_f16], mi355_dbscan_link[_f16]; host side and the finishing kernel in
// dbscan.hip): the self-join of the resident rows, a block of them as the GEMM's queries, swept twice.  A hit is the range
// search's: fp32 score >= roc_ceil_f32(threshold), NaN never, the row itself included.  Pass 1 counts each query row's hits
// (its degree); pass 2 joins core rows (degree >= min_samples) that hit each other in a union-find over parent[] and offers
// every core row to the non-core rows it hits or is hit by.  No pair list exists.  Every result is a sum of integers, a
// maximum of keys or the minimum row of a component: none depends on the order of the atomics, the query block or the tile cut.
// LDS of either epilogue: the degree epilogue's hit masks [128][4] u32 (the link epilogue's core flags are smaller)
constexpr size_t DBSCAN_EPI_BYTES = (size_t)128 * 4 * sizeof(unsigned);

// Pass 1: degree[row] += the row's hits in this tile, ONE integer atomic per (query row with hits, column tile)
struct DegreeEpi {
    float thr;                  // roc_ceil_f32(threshold)
    int* degree;                // [rows of this call]: the degrees of its queries (the host shifts it per query block)
    template <size_t STAGE> static constexpr size_t lds_bytes() {   // inside the staging buffers of every loop
        static_assert(STAGE >= DBSCAN_EPI_BYTES, "the degree epilogue would grow the GEMM's LDS");
        return STAGE;
    }
    // Scores are acc * ginv[col] as in the other epilogues: every hit is a hit of mi355_cosine_range on the same loop.
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const {
        const int Q = t.Q, m0 = t.m0;
        const i64 G = t.G, n0 = t.n0;
        constexpr int BM = 64 * MT;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
        unsigned* mask = reinterpret_cast<unsigned*>(smem);                  // [BM][4]: bit c % 32 of word c / 32 = column c
        // the hit masks as the range epilogue takes them: lanes 0-31 hold 32 consecutive columns of one row, lanes 32-63 those
        // of row + 4, so one ballot is two whole mask words; each (row, word) belongs to exactly one wave
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const i64 col = n0 + wn * 64 + j * 32 + lr;
            const float gs = (ginv && col < G) ? ginv[col] : 1.0f;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const bool hit = col < G && m0 + row < Q && acc[i][j][r] * gs >= thr;
                    const unsigned long long b = __ballot(hit);
                    if (lane == 0) {
                        mask[row * 4 + wn * 2 + j] = (unsigned)b;
                        mask[(row + 4) * 4 + wn * 2 + j] = (unsigned)(b >> 32);
                    }
                }
        }
        __syncthreads();
        if (tid < BM && m0 + tid < Q) {
            const int cnt = __popc(mask[tid * 4]) + __popc(mask[tid * 4 + 1]) + __popc(mask[tid * 4 + 2]) + __popc(mask[tid * 4 + 3]);
            if (cnt) atomicAdd(&degree[m0 + tid], cnt);
        }
    }
};

// The union-find of pass 2 lives in parent[N] (parent[x] == x: a root).  Other workgroups, on other XCDs, work on it during the
// same launch: the XCDs' L2s are not coherent and a CU's L1 is never refreshed, so inside the launch parent[] is read and
// written ONLY by agent-scope relaxed atomics (loads that bypass L1, a compare-and-swap; no plain access, no fence).
// Invariant: parent[x] <= x, and parent[x] is x itself or a true ancestor of x - a hook writes the smaller of two roots under
// the larger, a shortcut writes a value that an atomic load returned as the parent of x's parent.  A value read late is thus
// still an ancestor, and the compare-and-swap validates every hook against the word itself.
__device__ __forceinline__ int uf_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The root above x as this thread sees it, pointing every visited row at its grandparent.  The walk strictly descends
// (parent[y] < y unless y is a root), so it ends after at most x steps whatever other threads write meanwhile.
__device__ __forceinline__ int uf_find(int* parent, int x) {
    int p = uf_load(parent + x);
    while (p != x) {
        const int gp = uf_load(parent + p);
        // x is not a root and never becomes one again, so this store cannot undo a hook (hooks change roots only)
        if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}
// Joins the components of a and b: the larger root goes under the smaller, so a finished component's root is its smallest row
// in any order of the hooks.  Termination: the loop ends when both walks reach one root (nothing is written: in a dense
// cluster that is almost every hit) or when this thread's own compare-and-swap succeeds.  A failed one returns the word's
// value, a true ancestor below hi, and lo is below hi too: the next round's larger root is strictly smaller than this
// round's, so a thread makes fewer than N rounds.  No thread ever waits for a value another thread has yet to write.
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = seen;
        b = lo;
    }
}

// Pass 2, for every hit (i, j), i != j, of query row i = q0 + local row and column j: both core -> union(i, j); exactly one
// core -> the non-core row's border key takes the maximum with rank_composite(score_key(score), core row): the highest score
// wins, equal scores go to the lower core row.  degree[] is complete (pass 1 ended before this launch): plain loads.
struct LinkEpi {
    float thr;                  // roc_ceil_f32(threshold)
    int q0;                     // global row of this call's first query
    int min_samples;
    const int* degree;          // [G]
    int* parent;                // [G], see uf_find
    unsigned long long* border; // [G] keys, zeroed before the first call (every real score's key is > 0)
    template <size_t STAGE> static constexpr size_t lds_bytes() {   // inside the staging buffers of every loop
        static_assert(STAGE >= DBSCAN_EPI_BYTES, "the link epilogue would grow the GEMM's LDS");
        return STAGE;
    }
    // Scores are acc * ginv[col] as in the other epilogues: hits and border keys have the bits of mi355_cosine_range.
    template <int MT>
    __device__ __forceinline__ void tile(f32x16 (&acc)[MT][2], float* smem, const float* __restrict__ ginv, const TileCtx& t) const {
        const int Q = t.Q, m0 = t.m0;
        const i64 G = t.G, n0 = t.n0;
        constexpr int BM = 64 * MT;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
        unsigned char* ccore = reinterpret_cast<unsigned char*>(smem);      // [128] the tile's columns: 1 = core row
        unsigned char* qcore = ccore + RK_BN;                               // [BM] its query rows
        if (tid < RK_BN) ccore[tid] = n0 + tid < G && degree[n0 + tid] >= min_samples;
        if (tid >= 128 && tid - 128 < BM) qcore[tid - 128] = m0 + tid - 128 < Q && degree[q0 + m0 + tid - 128] >= min_samples;
        __syncthreads();
        // C[row = query][col = gallery]; lane: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = wn * 64 + j * 32 + lr;
            const i64 col = n0 + c;
            if (col < G) {
                const float gs = ginv ? ginv[col] : 1.0f;
                const bool cc = ccore[c];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        const float s = acc[i][j][r] * gs;
                        const int qi = q0 + m0 + row;
                        if (m0 + row >= Q || !(s >= thr) || qi == (int)col) continue;
                        const bool qc = qcore[row];
                        if (qc && cc) uf_union(parent, qi, (int)col);
                        else if (qc) atomicMax(&border[col], rank_composite(score_key(s), (unsigned)qi));
                        else if (cc) atomicMax(&border[qi], rank_composite(score_key(s), (unsigned)col));
                    }
            }
        }
    }
};

// Row norm of an fp32 row: one wave, float4 loads when vec (dim % 4 == 0 and 16-B aligned rows).  The lane-strided
// summation order is part of the result: every row normalisation of the library (mi355_l2_normalize_rows, the queries
// of every search, the fp16 gallery conversion) goes through this one function, so they give the same bits.
// The norm of a row with a NaN element is NaN and stays NaN, so the whole row comes out NaN, as x / max(|x|, eps) does in
// NumPy and torch (fmaxf(NaN, eps) is eps: it left such a row as x / eps around its NaN).  An Inf element: norm Inf, r = 0.
__device__ __forceinline__ float row_inv_norm(const float* __restrict__ x, int dim, float eps, int vec, int lane) {
    float ss = 0.f;
    if (vec) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        for (int i = lane; i < dim / 4; i += 64) {
            f32x4 v = x4[i];
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    } else {
        for (int i = lane; i < dim; i += 64) ss += x[i] * x[i];
    }
    ss = wave_sum(ss);
    const float norm = sqrtf(ss);
    return 1.0f / (norm < eps ? eps : norm);
}

// The fp32 row value x * r, then its rounding to fp16: two roundings, as l2_normalize_rows(x).half() does them (the fp16
// gallery conversion, rank_f16.hip, and the fp16 rows of the expansion, expand.hip).  (With
// -ffp-contract=fast, hipcc fuses the pair into v_fma_mixlo_f16, ONE rounding of the exact product, which differs in the
// last bit now and then; `#pragma clang fp contract(off)` does not stop that backend fold.  The empty asm only pins the
// fp32 product in a register - it emits no instruction.)
__device__ __forceinline__ _Float16 scaled_f16(float x, float r) {
    float p = x * r;
    asm volatile("" : "+v"(p));
    return (_Float16)p;
}

// The last step of every kernel that makes normalised rows from fp32 sums (the expansion, expand.hip; the whitening
// transform, whiten.hip): one wave takes the norm of the fp32 row x[dim] as l2_normalize_rows does (VEC: dim % 4 == 0, rows
// 16-byte aligned), then scales x in place (fp32 output: x IS the output row) or stores fp16(x * r) into y[ld] with elements
// dim .. ld-1 zeroed (the mi355_gallery_to_f16 row).
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
template <bool VEC, bool OF16>
__device__ __forceinline__ void normalize_row_store(float* x, _Float16* y, int dim, int ld, float eps, int lane) {
    const int nu = VEC ? dim / 4 : dim;
    const float r = row_inv_norm(x, dim, eps, VEC ? 1 : 0, lane);
    if constexpr (!OF16) {
        if constexpr (VEC) {
            f32x4* x4 = reinterpret_cast<f32x4*>(x);
            for (int i = lane; i < nu; i += 64) {
                f32x4 v = x4[i];
                v.x *= r; v.y *= r; v.z *= r; v.w *= r;
                x4[i] = v;
            }
        } else {
            for (int i = lane; i < dim; i += 64) x[i] = x[i] * r;
        }
    } else {
        if constexpr (VEC) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
            for (int i = lane; i < ld / 4; i += 64) {
                f16x4_t h = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
                if (i < nu) {
                    const f32x4 v = x4[i];
                    h = (f16x4_t){scaled_f16(v.x, r), scaled_f16(v.y, r), scaled_f16(v.z, r), scaled_f16(v.w, r)};
                }
                reinterpret_cast<f16x4_t*>(y)[i] = h;
            }
        } else {
            for (int i = lane; i < ld; i += 64) y[i] = i < dim ? scaled_f16(x[i], r) : (_Float16)0.f;
        }
    }
}

static inline int vec_ok(const void* p, int dim) { return (dim % 4 == 0) && (((uintptr_t)p & 15) == 0); }

// ---- host side of the selection (rank.hip)
constexpr int SMALL_K = 8;          // k <= SMALL_K: per-thread sorted lists; the fused GEMM epilogue selects up to this k
constexpr int LARGE_K = 1024;       // largest k of any search

// Scratch of topk_select for Q rows of rowlen candidates.
size_t topk_ws_bytes(i64 Q, i64 G, int k);
// Top-k of each row of vals[Q][rowlen] (implicit indices j + idx_offset, explicit int64 idxs, or the fused epilogue's int32
// local indices idxs32 with IDX32_PAD = missing) into out_val / out_idx [Q][k].
// filt (filtered searches): with implicit indices the first level reads an ineligible candidate as a pad; either way the
// pads left in the output (fewer than k eligible rows) become (-inf, -1).
int topk_select(const float* vals, const i64* idxs, i64 Q, i64 rowlen, i64 in_stride, int k, i64 idx_offset, float* out_val,
                i64* out_idx, void* ws, size_t ws_bytes, hipStream_t st, const int* idxs32 = nullptr,
                const RankFilter* filt = nullptr);
// The filter of the query block starting at query q0
RankFilter filter_from(const RankFilter& f, i64 q0);
// Checks a mi355_rank_filter and turns it into a RankFilter for a search with idx_offset
int make_filter(const mi355_rank_filter* f, i64 idx_offset, const char* who, RankFilter* out);
// Which branch the calling thread's last search took (mi355_rank_last_path)
void set_rank_path(int path);
// Whether a (Q, G, k) search selects inside the GEMM epilogue (k <= SMALL_K, Q > 4), and how many queries one GEMM call
// takes so that the candidate lists / the score slab stay bounded.
bool fused_select(i64 Q, i64 G, int k);
i64 query_block(i64 Q, i64 G, int k);
// Resident workgroups per CU x CUs of the current device for one kernel (sets its dynamic LDS limit; cached per device).
int kernel_slots(const void* fn, size_t lds, int* cache, int* slots_out);
// Column tiles of a GEMM's main launch of whole rounds (the rest go to a tail launch of 64-row tiles).
int whole_round_tiles(int ntx, int ny, int slots);
// The slots a GEMM call is cut by: the device's own count, or the calling thread's test override (mi355_rank_set_round_slots)
int round_slots(int device_slots);
// The cut of the calling thread's last GEMM call (mi355_rank_last_tiles)
void set_last_tiles(int slots, int ny, int main_tiles, int tail_tiles, int tail_ny);

// ---- host side of the tiled cosine GEMMs: exact fp32, split bf16 (rank.hip: F32Gemm, SplitGemm, PreparedGemm) and fp16 and
// int8 rows (rows_gemm.h: RowsGemm<F16Rows>, RowsGemm<I8Rows>).  A family F supplies only what differs between them:
//   F::stage_bytes<MT>()             the LDS of its staging buffers
//   F::kernel<MT, Epi>()             its kernel with epilogue Epi
//   F::launch<MT, Epi>(...)          one launch of that kernel over column tiles [x0, x0 + xtiles) x ny query tiles
// Per loop two kernels exist: k_*<MT, FK> for the unfiltered slab (FK = 0) and selection (the names profiles are keyed by), and
// k_*_epi<MT, Epi> for every other epilogue.  Both take the epilogue as their last argument.
template <int FK> using PlainEpi = std::conditional_t<FK == 0, SlabEpi, SelectEpi<(FK > 0 ? FK : 1), false>>;
template <class Epi> constexpr int plain_fk = -1;              // FK of the k_*<MT, FK> kernel that runs Epi; -1: k_*_epi<MT, Epi>
template <> inline constexpr int plain_fk<SlabEpi> = 0;
template <int FK> constexpr int plain_fk<SelectEpi<FK, false>> = FK;
template <class Epi> constexpr bool is_select = false;         // the fused selection (MI355_RANK_PATH_FUSED)
template <int FK, bool FILT> constexpr bool is_select<SelectEpi<FK, FILT>> = true;
template <int FK, bool FILT> constexpr bool is_select<AdjSelectEpi<FK, FILT>> = true;
static_assert(sizeof(SelectEpi<1, true>) == 2 * sizeof(int) + 2 * sizeof(void*) + sizeof(RankFilter),
              "the unadjusted selection's kernel argument keeps its layout");

// What every GEMM call over Q queries shares; the epilogue object travels beside it
struct TileArgs {
    const void* qry;            // the queries as the family reads them: fp32 rows, bf16 split planes, fp16 or int8 planes
    const void* gal;            // the gallery: fp32 rows, bf16 planes (prepared), fp16 rows or int8 codes
    const float* ginv;          // 1 / |gallery row| (fp32 rows), the rows' scales (int8 codes), or null
    int Q;
    i64 G;
    int D;                      // dim (fp16 / int8 rows: their padded length ld)
};

// Column tiles [x0, ntx) of a GEMM call.
// Wave quantisation: 1564 tiles on 768 slots run as 2.04 rounds and the 28 tiles of the third round cost a whole round
// (0.15 ms of 0.83 at Q=256 x 100k on the fp32 loop).  At MT = 2 whole rounds go out as 128-row tiles and the remaining
// column tiles as a second launch of 64-row tiles (same column tiles, same k order: every score is bit-identical), which
// halves the tiles' length and doubles their number.
template <class F, int MT, class Epi>
int launch_tiles(const TileArgs& a, const Epi& epi, hipStream_t st, int x0 = 0, bool tail = false) {
    constexpr size_t lds = Epi::template lds_bytes<F::template stage_bytes<MT>()>();
    static int cache[MI355_MAX_DEVICES] = {0};   // per instantiation: hipFuncSetAttribute once per device
    int slots = 0;
    if (int e = kernel_slots((const void*)F::template kernel<MT, Epi>(), lds, cache, &slots)) return e;
    const int ntx = cdiv(a.G, RK_BN), ny = cdiv(a.Q, 64 * MT);
    if (!tail) slots = round_slots(slots);
    const int x1 = MT == 2 ? whole_round_tiles(ntx, ny, slots) : ntx;
    if (!tail) set_last_tiles(slots, ny, x1, ntx - x1, x1 < ntx ? cdiv(a.Q, 64) : 0);
    if (x1 > x0) {
        F::template launch<MT, Epi>(dim3((unsigned)(x1 - x0) * (unsigned)ny), lds, st, a, epi, x0, ntx, x1 - x0, ny);
        MI355_LAUNCH_CHECK();
    }
    if constexpr (MT == 2) {
        if (x1 < ntx) return launch_tiles<F, 1, Epi>(a, epi, st, x1, true);
    }
    return OK;
}
// A GEMM call of family F: 128-query tiles above 64 queries, 64-query tiles otherwise
template <class F, class Epi>
int cos_gemm_tiles(const TileArgs& a, const Epi& epi, hipStream_t st) {
    return a.Q > 64 ? launch_tiles<F, 2, Epi>(a, epi, st) : launch_tiles<F, 1, Epi>(a, epi, st);
}

// fn(the fused selection's epilogue for k): it keeps FK >= k candidates per (query, column tile)
template <bool FILT, class Fn>
int with_select_epi(int k, float* cand_val, int* cand_idx, const RankFilter& f, Fn&& fn) {
    if (k <= 1) return fn(SelectEpi<1, FILT>{{k, cand_val, cand_idx, f, {}}});
    if (k <= 2) return fn(SelectEpi<2, FILT>{{k, cand_val, cand_idx, f, {}}});
    if (k <= 4) return fn(SelectEpi<4, FILT>{{k, cand_val, cand_idx, f, {}}});
    return fn(SelectEpi<8, FILT>{{k, cand_val, cand_idx, f, {}}});
}
// The same with the map of adj (this call's queries) in front of the selection
template <bool FILT, class Fn>
int with_adjusted_select_epi(int k, float* cand_val, int* cand_idx, const RankFilter& f, const ScoreAdjust& adj, Fn&& fn) {
    if (k <= 1) return fn(AdjSelectEpi<1, FILT>{{k, cand_val, cand_idx, f, adj}});
    if (k <= 2) return fn(AdjSelectEpi<2, FILT>{{k, cand_val, cand_idx, f, adj}});
    if (k <= 4) return fn(AdjSelectEpi<4, FILT>{{k, cand_val, cand_idx, f, adj}});
    return fn(AdjSelectEpi<8, FILT>{{k, cand_val, cand_idx, f, adj}});
}

// ---- host side of the ROC entries (roc.cpp)
// Checks T thresholds (host float64: count, finite, ascending) and fills the binning plan of a (null: checks only)
int roc_check_thresholds(const double* thr, int T, const char* who, RocArgs* a);
// Checks the label / exclude pointers and hist of mi355_roc_pairs_hist[_f16] and fills them into a
int roc_check_pairs(const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude, int64_t idx_offset,
                    const double* thresholds_dev, int64_t* hist, const char* who, RocArgs* a);
// The block of queries [q0, ...) of a
RocArgs roc_from(const RocArgs& a, i64 q0);
// Queries per GEMM call of a histogram (no slab, no candidates: only the grid size bounds it)
i64 roc_query_block(i64 Q, i64 G);

// ---- one top-k search (mi355_rank_topk[_filtered], mi355_rank_topk_prepared, mi355_rank_topk_f16[_filtered])
// Scratch of a search, carved from the caller's workspace (ws null: sizes only, total = the bytes it needs).
struct RankWs {
    float* qn; void* qs; float* ginv; float* S; float* cand_val; int* cand_idx; void* topk; size_t topk_bytes; size_t total;
};
// qs: planes_bytes(queries of one GEMM call, D) bytes for the queries' planes (null: none); need_S = false: no selection
// (mi355_cosine_scores, k = 0)
RankWs carve(void* ws, i64 Q, i64 G, int D, int k, size_t (*planes_bytes)(i64, int), bool need_ginv, bool need_S = true);
// "rank/normalize": the queries into w.qn and, with a gallery, 1 / |row| of its rows into w.ginv
int normalize_search(const float* queries, i64 Q, const float* gallery, i64 G, int dim, float eps, const RankWs& w,
                     hipStream_t st);

// fn(the epilogue of one GEMM call of a top-k search over the scratch w): the fused per-tile lists cand_val / cand_idx
// [Q][cdiv(G, 128)][k], filtered by f (null: unfiltered), or the score slab S [Q][G] (unfiltered: topk_select filters it)
template <class Fn>
int with_topk_epi(const RankWs& w, int k, const RankFilter* f, Fn&& fn) {
    if (!w.cand_val) return fn(SlabEpi{w.S});
    if (f) return with_select_epi<true>(k, w.cand_val, w.cand_idx, *f, fn);
    return with_select_epi<false>(k, w.cand_val, w.cand_idx, RankFilter{}, fn);
}

// Normalises the queries, then per block of query_block(Q, G, k) queries: score(q0, qn, f) writes the fused per-tile lists
// (fused_select) or the score slab of queries [q0, q0 + qn) (f: their filter, or null), and topk_select merges them into
// rows [q0, q0 + qn) of out_val / out_idx.  slab_range: roctx range around the top-k of a slab (null: none).
template <class Score>
int search_blocks(const float* queries, const float* gallery_to_norm, i64 Q, i64 G, int dim, int k, float eps, i64 idx_offset,
                  const RankFilter* filt, float* out_val, i64* out_idx, const RankWs& w, hipStream_t st, const char* slab_range,
                  Score&& score) {
    if (int e = normalize_search(queries, Q, gallery_to_norm, G, dim, eps, w, st)) return e;
    const bool fused = fused_select(Q, G, k);
    const i64 qb = query_block(Q, G, k), rowlen = fused ? cdiv(G, RK_BN) * (i64)k : G;
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = (Q - q0 < qb) ? Q - q0 : qb;
        const RankFilter fb = filt ? filter_from(*filt, q0) : RankFilter{};
        const RankFilter* f = filt ? &fb : nullptr;
        if (int e = score(q0, qn, f)) return e;
        if (!fused && k > SMALL_K) set_rank_path(mi355_rank_last_path() | MI355_RANK_PATH_BITONIC);
        RoctxRange range(fused ? "rank/merge candidates" : slab_range);
        if (int e = topk_select(fused ? w.cand_val : w.S, nullptr, qn, rowlen, rowlen, k, idx_offset, out_val + q0 * k,
                                out_idx + q0 * k, w.topk, w.topk_bytes, st, w.cand_idx, f))
            return e;
    }
    return OK;
}

// ---- host side of the range search (range.hip)
// Workspace of mi355_cosine_range[_f16]: the CSR offsets [Q + 1] first (mi355_range_compact finds them there), the call's
// hit cursor, the search's own scratch (carve: normalised queries, planes of one GEMM call, 1 / |row|), then the
// (query, tile) table and the row counts of one query block.  ws null: sizes only.
struct RangeWs {
    i64* offsets; unsigned long long* cursor; RankWs w; i64* tstart; int* tcount; i64* rowcnt; size_t total;
};
RangeWs range_carve(void* ws, i64 Q, i64 G, int D, size_t (*planes_bytes)(i64, int), bool need_ginv);
// Queries per GEMM call of a range search: the (query, tile) table of one call stays around 100 MB
i64 range_query_block(i64 Q, i64 G);
// The checks every range search shares (before any HIP call); fills *f from filter (null: no filter)
int range_check(const void* queries, i64 Q, const void* gallery, i64 G, int dim, double threshold,
                const mi355_rank_filter* filter, i64 idx_offset, void* candidates, i64 capacity, const int64_t* nnz,
                const char* who, RankFilter* f);
// Q = 0 or G = 0: all-zero offsets, no hit
int range_empty(const RangeWs& w, i64 Q, int64_t* nnz, hipStream_t st);
// The compaction of one query block [q0, q0 + qn) whose hits begin at CSR position off: row counts, offsets, then every
// (query, tile) chunk of raw copied in tile order to canon[offsets[q] ...]
int range_compact_block(const RangeWs& w, i64 q0, i64 qn, i64 G, i64 off, const unsigned long long* raw,
                        unsigned long long* canon, hipStream_t st);

// ---- host side of the full-gallery ranks (ranks.hip)
// The checks mi355_rank_positives[_f16] share (before any HIP call); fills *a
int ranks_check(const void* queries, i64 Q, const void* gallery, i64 G, int dim, const int64_t* query_labels,
                const int64_t* gallery_labels, const int64_t* exclude, i64 idx_offset, const int64_t* offsets,
                const int64_t* offsets_host, const void* pos_keys, i64 nnz, const void* before, i64 query_block, const char* who,
                RanksArgs* a);
// The block of queries [q0, ...) of a
RanksArgs ranks_from(const RanksArgs& a, i64 q0);
// Queries per GEMM call of the counting pass: roc_query_block, or the caller's smaller query_block (> 0)
i64 ranks_query_block(i64 Q, i64 G, i64 query_block);


// ---- the searches without a top-k (ROC histogram, range, ranks) exist once for both kinds of gallery rows (rank.hip)
// The gallery as a search reads it: fp32 rows [G][dim], the fp16 rows of mi355_gallery_to_f16, the int8 codes and scales
// of mi355_gallery_to_i8, or the fp4 codes and multipliers of mi355_gallery_to_fp4
struct GalleryRows {
    const float* f32;           // fp32 rows, or null
    bool unit;                  // fp32 rows: unit length already (no 1 / |row| pass); fp16 and int8 rows always are
    const void* f16;            // fp16 rows [G][ld], or null
    int ld;                     // the padded length of fp16 / int8 rows, the bytes of an fp4 row
    size_t (*planes_bytes)(i64, int);   // bytes of the operand the GEMM reads for (queries of one call, dim)
    const void* i8 = nullptr;   // int8 codes [G][ld], or null
    const float* scales = nullptr;      // their scales [G] (fp4 rows: their multipliers)
    const void* fp4 = nullptr;  // packed e2m1 codes [G][ld] of mi355_gallery_to_fp4, or null
    const void* rows() const { return fp4 ? fp4 : i8 ? i8 : f16 ? f16 : (const void*)f32; }
};
// One GEMM call over fp16 rows: the normalised queries qn [Q][dim] into their fp16 planes qs, then RowsGemm<F16Rows> with epi;
// sets the rank path (rank_f16.hip; instantiated there for the epilogues of the three searches below)
template <class Epi>
int cos_gemm_f16(const void* rows, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi, hipStream_t st);
// The same over int8 rows: the queries' two int8 planes and s_q into qs, then RowsGemm<I8Rows> with epi (rank_i8.hip;
// instantiated there for the range epilogue)
template <class Epi>
int cos_gemm_i8(const void* codes, const float* scales, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                hipStream_t st);
// The same over fp4 rows: the queries' two e2m1 planes and s_q into qs, then RowsGemm<Fp4Rows> with epi (rank_fp4.hip;
// instantiated there for the range epilogue)
template <class Epi>
int cos_gemm_fp4(const void* codes, const float* mults, int ld, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                 hipStream_t st);
// mi355_roc_pairs_hist[_f16] under the name who; need: the entry's workspace size
int roc_pairs_hist(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, const int64_t* query_labels,
                   const int64_t* gallery_labels, const int64_t* exclude, i64 idx_offset, const double* thresholds,
                   const double* thresholds_dev, int T, int64_t* hist, void* workspace, size_t workspace_bytes, size_t need,
                   void* stream, const char* who);
// mi355_cosine_range[_f16] and, with keep_all (every eligible pair is a hit), mi355_positives_range[_f16]
int cosine_range(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, double threshold, i64 idx_offset,
                 const mi355_rank_filter* filter, void* candidates, i64 capacity, int64_t* nnz, void* workspace,
                 size_t workspace_bytes, void* stream, bool keep_all, const char* who);
// mi355_rank_positives[_f16]
int rank_positives(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, const int64_t* query_labels,
                   const int64_t* gallery_labels, const int64_t* exclude, i64 idx_offset, const int64_t* offsets,
                   const int64_t* offsets_host, const uint64_t* pos_keys, i64 nnz, uint32_t* before, i64 query_block,
                   void* workspace, size_t workspace_bytes, size_t need, void* stream, const char* who);
// mi355_rank_topk_adjusted[_f16] (k >= 1: out_val / out_idx [Q][k]) and mi355_cosine_scores_adjusted[_f16] (k = 0: out_val is the
// slab [Q][G], out_idx unused): the search of mi355_rank_topk_filtered over t = s * (aq + ag) - (bq + bg).  Every Q runs on the
// tiles (no GEMV), a prepared gallery on its fp32 rows.  query_block > 0: at most that many queries per GEMM call.
// workspace = carve(Q, G, dim, k, planes, need_ginv, k > 0).  Arguments checked by adjust_check (scorenorm.hip).
GalleryRows f32_rows(const float* gallery, int is_normalized);
int adjusted_search(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, int k, i64 idx_offset,
                    const ScoreAdjust& adj, const RankFilter* filt, i64 query_block, float* out_val, i64* out_idx, void* workspace,
                    size_t workspace_bytes, hipStream_t st, const char* who);
// The checks the adjusted entries share, before any HIP call; fills *adj and, with a filter, *f
int adjust_check(const void* queries, i64 Q, const GalleryRows& g, i64 G, int dim, int k, bool topk, const mi355_score_adjust* adjust,
                 const mi355_rank_filter* filter, i64 idx_offset, i64 query_block, const void* out_val, const void* out_idx,
                 const char* who, ScoreAdjust* adj, RankFilter* f);
// mi355_nearest_centroid[_f16]: workspace = the keys best[G], then carve(K, G, dim, 0, planes, need_ginv).  need_ginv: room
// for 1 / |row| of fp32 rows that are not normalised (the fp32 sizer always counts it: it does not know the rows).
size_t nearest_ws_bytes(i64 K, i64 G, int dim, size_t (*planes_bytes)(i64, int), bool need_ginv);
int nearest_centroid(const float* centroids, i64 K, const GalleryRows& g, i64 G, int dim, float eps, i64 query_block,
                     int64_t* assign, float* score, void* workspace, size_t workspace_bytes, void* stream, const char* who);

// mi355_dbscan_degree[_f16] (link false: parent / border unused) and mi355_dbscan_link[_f16]: one sweep of queries
// [q0, q0 + rows) of the self-join over the N rows of g.  workspace = carve(rows, N, dim, 0, planes, need_ginv)
size_t dbscan_ws_bytes(i64 rows, i64 N, int dim, size_t (*planes_bytes)(i64, int), bool need_ginv);
int dbscan_sweep(const float* queries, i64 q0, i64 rows, const GalleryRows& g, i64 N, int dim, float eps, double threshold,
                 int min_samples, int32_t* degree, int32_t* parent, uint64_t* border, bool link, void* workspace,
                 size_t workspace_bytes, void* stream, const char* who);
// The checks both sweeps share (dbscan.hip), before any HIP call
int dbscan_check(const void* queries, i64 q0, i64 rows, const void* gallery, i64 N, int dim, double threshold, int min_samples,
                 const void* degree, const void* parent, const void* border, bool link, const char* who);

// ---- mi355_cluster_members without its host sync (kmeans.hip), for the IVF scan (ivf.hip): offsets [K + 1] and order [N] of
// assign [N]; *flag: a device word that is 1 after a value outside [0, K) (such a value is in no cluster).  workspace:
// members_ws_bytes(N, K) bytes.  N >= 1, 1 <= K < 2^24.
size_t members_ws_bytes(i64 N, i64 K);
int members_async(const int64_t* assign, i64 N, i64 K, int64_t* offsets, int64_t* order, void* workspace, hipStream_t st,
                  const unsigned** flag);

}  // namespace mi355
