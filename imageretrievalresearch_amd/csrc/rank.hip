// Rank half of the hot path: row normalisation, cosine GEMM with fused top-k selection, shard merge, pair cosine,
// ContrastiveLoss, hit counting.  gfx950 only.
//
// Reference semantics: torch.nn.CosineSimilarity(dim=1, eps=1e-6) + torch.topk as called at
// train/train.py:250-251 (see include/mi355_retrieval.h).  Inputs, norms, accumulation and scores are fp32.  The
// GEMM has two loops with the same tiling and epilogue:
//   * default: fp32 operands split into three bf16 planes, six of the nine bf16 products per element on
//     v_mfma_f32_32x32x16_bf16 with fp32 accumulation (k_cos_gemm_split; error per product <= 2^-23, the size of the
//     one rounding an fmaf spends - measured as close to the float64 cosine as the exact loop, ~1e-7);
//   * MI355_RANK_EXACT_F32=1, gallery rows not 16-byte aligned, or Q <= 4 (GEMV): v_mfma_f32_32x32x2_f32 / fmaf, bit-for-bit
//     an fp32 fmaf chain (2.7x the matrix-pipe time).
// Either way an index can only differ from the CPU oracle where two scores are closer than fp32 summation noise.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <limits.h>
#include <stdlib.h>
#include <math.h>

namespace mi355 {

// =====================================================================================
// row norms
// =====================================================================================
// One wave per row; float4 loads when dim % 4 == 0 and rows are 16-B aligned.
template <bool WRITE_ROWS>
__global__ __launch_bounds__(256) void k_row_norm(const float* __restrict__ in, float* __restrict__ out,
                                                  float* __restrict__ inv, i64 rows, int dim, float eps,
                                                  int vec) {
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = in + row * dim;
    const float r = row_inv_norm(x, dim, eps, vec, lane);
    if (inv != nullptr && lane == 0) inv[row] = r;
    if (WRITE_ROWS) {
        float* y = out + row * dim;
        if (vec) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
            f32x4* y4 = reinterpret_cast<f32x4*>(y);
            for (int i = lane; i < dim / 4; i += 64) {
                f32x4 v = x4[i];
                v.x *= r; v.y *= r; v.z *= r; v.w *= r;
                y4[i] = v;
            }
        } else {
            for (int i = lane; i < dim; i += 64) y[i] = x[i] * r;
        }
    }
}

// =====================================================================================
// top-k selection
// =====================================================================================
// (the ordering of (score, index) candidates, better(), lives in rank_common.h: the PQ scan selects with it too)

// =====================================================================================
// fp32 operands on the bf16 matrix pipe: three-way split, six products
// =====================================================================================
// x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (round-to-nearest-even; both subtractions are exact
// in fp32, and |x - h - m - l| <= 2^-25 |x|: the three 8-bit significands cover fp32's 24).  A product x*y is then the sum
// of nine bf16 x bf16 products, each EXACT in the fp32 accumulator; the kernel keeps the six largest
//     h*h' + (h*m' + m*h') + (h*l' + l*h' + m*m')
// and drops m*l', l*m', l*l' (<= 2^-24 |x*y| each, either sign).  Per product that is the size of ONE fp32 rounding -
// what the exact-fp32 MFMA (an fmaf chain) spends on every product anyway - so scores agree with the fp32 chain to
// ~1e-7 (measured against the fp64 oracle in tests/test_rank_gpu.py); the accumulation itself stays fp32.  Six
// v_mfma_f32_32x32x16_bf16 do the work of eight v_mfma_f32_32x32x2_f32 in 3/8 of the matrix-pipe time (192 vs 512 cycles).
// NaN / Inf inputs give NaN scores (Inf - Inf in the split), which the selection orders as torch.topk does.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = pack2bf(x0, x1);
    const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
    m = pack2bf(r0, r1);
    l = pack2bf(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xffff0000u));
}
__device__ __forceinline__ void split3(const f32x4 a, const f32x4 b, u32x4& h, u32x4& m, u32x4& l) {
    unsigned hh[4], mm[4], ll[4];
    split3_pair(a.x, a.y, hh[0], mm[0], ll[0]);
    split3_pair(a.z, a.w, hh[1], mm[1], ll[1]);
    split3_pair(b.x, b.y, hh[2], mm[2], ll[2]);
    split3_pair(b.z, b.w, hh[3], mm[3], ll[3]);
    h = (u32x4){hh[0], hh[1], hh[2], hh[3]};
    m = (u32x4){mm[0], mm[1], mm[2], mm[3]};
    l = (u32x4){ll[0], ll[1], ll[2], ll[3]};
}

// Normalised queries -> split planes in MFMA-fragment order: Qs[row block of 32][k step of 16][plane h,m,l][lane][8 bf16],
// lane = row + 32 * (k half): every (row block, k step, plane) is 1 KB that one global_load_lds moves into LDS exactly as
// the A operand of v_mfma_f32_32x32x16_bf16 wants it (lane-linear ds_read_b128, no padding, no swizzle).  Rows >= Q and
// k >= D are zero.  A 256-byte zero page follows the planes (source of the GEMM's out-of-range gallery loads).
__global__ __launch_bounds__(256) void k_split_queries(const float* __restrict__ Qn, bf16_t* __restrict__ Qs, int Q, int D,
                                                       int n_steps, int n_frag) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);   // fragment = (row block, k step)
    if (blockIdx.x == 0 && threadIdx.x < 64) reinterpret_cast<unsigned*>(Qs + (size_t)n_frag * 3 * 512)[threadIdx.x] = 0u;   // zero page
    if (f >= n_frag) return;
    const int lane = threadIdx.x & 63;
    const int rb = f / n_steps, s = f % n_steps;
    const int row = rb * 32 + (lane & 31), k0 = s * 16 + (lane >> 5) * 8;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (row < Q && k0 + e < D) ? Qn[(i64)row * D + k0 + e] : 0.f;
    u32x4 h, m, l;
    split3((f32x4){x[0], x[1], x[2], x[3]}, (f32x4){x[4], x[5], x[6], x[7]}, h, m, l);
    u32x4* o = reinterpret_cast<u32x4*>(Qs + (size_t)f * 3 * 512) + lane;
    o[0] = h; o[64] = m; o[128] = l;
}

// =====================================================================================
// cosine GEMM:  S[q][g] = sum_d Qn[q][d] * Gal[g][d] * (ginv ? ginv[g] : 1)
// =====================================================================================
// Block = 4 waves as 2(M) x 2(N); wave tile = (MT*32) queries x 64 gallery rows; block tile =
// (64*MT) x 128 x BK.  Both operands are "row x k-contiguous", so they share one LDS image:
// [rows][BK + 4] floats (the 4-float pad makes ds_read_b128 of 16 distinct rows bank-conflict free).
// Per lane a float4 at k = 8t + 4*(lane>>5) feeds four 32x32x2 k-steps; A and B use the same k
// permutation, which only reorders the (exact) fma chain.
template <int MT, int RK_BK, bool VEC, class Epi>
__device__ __forceinline__ void cos_gemm_f32_tile(const float* __restrict__ Qn, const float* __restrict__ Gal,
                                                  const float* __restrict__ ginv, int Q, i64 G, int D, int x0, int ntx,
                                                  int xtiles, int ny, const Epi& epi) {
    // x0 / ntx: this launch covers the column tiles [x0, x0 + xtiles) of ntx for ny query blocks (the host splits a call into a main launch
    // of whole rounds and a tail launch of smaller tiles)
    constexpr int BM = 64 * MT;
    constexpr int RK_LD = RK_BK + 4;      // +4 floats: ds_read_b128 of 16 distinct rows is bank-conflict free (36 and 20)
    constexpr int CPR = RK_BK / 4;        // float4 columns per row of a K-tile
    constexpr int RPP = 256 / CPR;        // rows covered by one pass of the 256 threads
    constexpr int A_LOADS = BM / RPP;     // float4 loads per thread per K-tile for A
    constexpr int B_LOADS = RK_BN / RPP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [2][BM][RK_LD]
    float* Bs = smem + 2 * BM * RK_LD;         // [2][RK_BN][RK_LD]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by;
    rank_tile_of((int)blockIdx.x, xtiles, ny, bx, by);
    const i64 n0 = (i64)(bx + x0) * RK_BN;
    const int m0 = by * BM;

    const int c4 = tid % CPR;  // float4 column within the K-tile
    const int r0 = tid / CPR;

    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4 ra[A_LOADS], rb[B_LOADS];

    auto load_tile = [&](int k0) {
        const int k = k0 + c4 * 4;
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const int row = m0 + r0 + RPP * i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < Q) {
                const float* p = Qn + (i64)row * D + k;
                if (VEC) {
                    if (k + 3 < D) v = *reinterpret_cast<const f32x4*>(p);
                } else {
                    if (k + 0 < D) v.x = p[0];
                    if (k + 1 < D) v.y = p[1];
                    if (k + 2 < D) v.z = p[2];
                    if (k + 3 < D) v.w = p[3];
                }
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const i64 row = n0 + r0 + RPP * i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < G) {
                const float* p = Gal + row * D + k;
                if (VEC) {
                    if (k + 3 < D) v = *reinterpret_cast<const f32x4*>(p);
                } else {
                    if (k + 0 < D) v.x = p[0];
                    if (k + 1 < D) v.y = p[1];
                    if (k + 2 < D) v.z = p[2];
                    if (k + 3 < D) v.w = p[3];
                }
            }
            rb[i] = v;
        }
    };
    auto store_tile = [&](int buf) {
        float* a = As + buf * BM * RK_LD;
        float* b = Bs + buf * RK_BN * RK_LD;
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i)
            *reinterpret_cast<f32x4*>(a + (r0 + RPP * i) * RK_LD + c4 * 4) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i)
            *reinterpret_cast<f32x4*>(b + (r0 + RPP * i) * RK_LD + c4 * 4) = rb[i];
    };

    const int nt = (D + RK_BK - 1) / RK_BK;
    load_tile(0);
    store_tile(0);
    __syncthreads();

    const int lr = lane & 31;
    const int lk = (lane >> 5) * 4;
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) load_tile((t + 1) * RK_BK);
        const float* a = As + buf * BM * RK_LD + (wm * MT * 32 + lr) * RK_LD + lk;
        const float* b = Bs + buf * RK_BN * RK_LD + (wn * 64 + lr) * RK_LD + lk;
#pragma unroll
        for (int t8 = 0; t8 < RK_BK / 8; ++t8) {
            f32x4 af[MT], bfr[2];
#pragma unroll
            for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const f32x4*>(a + i * 32 * RK_LD + t8 * 8);
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = *reinterpret_cast<const f32x4*>(b + j * 32 * RK_LD + t8 * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bfr[j][e], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nt) store_tile(buf ^ 1);
        __syncthreads();
    }

    epi.tile(acc, smem, ginv, TileCtx{Q, G, ntx, n0, m0});
}
template <int MT, int RK_BK, bool VEC, int FK>
__global__ __launch_bounds__(256) void k_cos_gemm(const float* __restrict__ Qn, const float* __restrict__ Gal,
                                                  const float* __restrict__ ginv, int Q, i64 G, int D, int x0, int ntx,
                                                  int xtiles, int ny, PlainEpi<FK> epi) {
    cos_gemm_f32_tile<MT, RK_BK, VEC>(Qn, Gal, ginv, Q, G, D, x0, ntx, xtiles, ny, epi);
}
// Every other epilogue (filtered selection, histogram, range, ranks): the same loop
template <int MT, int RK_BK, bool VEC, class Epi>
__global__ __launch_bounds__(256) void k_cos_gemm_epi(const float* __restrict__ Qn, const float* __restrict__ Gal,
                                                      const float* __restrict__ ginv, int Q, i64 G, int D, int x0, int ntx,
                                                      int xtiles, int ny, Epi epi) {
    cos_gemm_f32_tile<MT, RK_BK, VEC>(Qn, Gal, ginv, Q, G, D, x0, ntx, xtiles, ny, epi);
}

// =====================================================================================
// The same GEMM on the bf16 matrix pipe (three-way split, six products; see split3 above).  Same block / wave tiling and
// the same epilogues as k_cos_gemm; one 32x32x16 k-step per K-tile.  Both operands arrive by LDS-DMA, the loop is dma_ring
// (rank_common.h): no load has a register destination, one counted wait and one LDS-only barrier per k-step.  (With
// register-staged B loads hipcc drained the vector-memory counter before every store to LDS.)
//   A (queries): pre-split planes in fragment order (k_split_queries), 1 KB per (row block, plane), from L2.
//   B (gallery): from HBM, two k-steps ahead.  A B operand type says how it arrives and how a wave's 32-row fragment j
//     becomes its planes (h, m, l):
//       WAVE_PIECES, STAGE_BYTES   DMA pieces per wave and bytes per ring stage of a k-step
//       init(...)                  the lane's source and LDS addresses for the tile at gallery row n0
//       dma(Bs, stage, t, swave)   issues the wave's pieces of k-step t (past the end too: the count in flight stays uniform)
//       read(Bs, stage, j)         the lane's Frag out of LDS;  planes(Frag) its Planes3
//       SPLITS                     planes() is VALU work, to be interleaved with the MFMAs
// =====================================================================================
// A ring: 2 stages at MT = 2 (one k-step ahead; a third stage would cost the split kernel its third workgroup per CU), 3
// stages at MT = 1 (two k-steps ahead: the 64-row tiles are the tail launch and the small-Q shapes, few workgroups per CU
// with nothing else to hide a piece's latency behind)
template <int MT> constexpr int SPLIT_A_RING = MT == 1 ? 3 : 2;
template <int MT> constexpr size_t SPLIT_A_BYTES = (size_t)SPLIT_A_RING<MT> * (64 * MT / 32) * 3 * 1024;
struct Planes3 {
    bf16x8 h, m, l;
};

// fp32 rows with 16-byte aligned rows (D % 4 == 0; other shapes stay on the fp32 loop): a piece is 16 rows x 64 B, wave w
// moves pieces 2w and 2w + 1 (lane -> row 16 * piece + lane / 4, position lane % 4).  The 16-byte chunk c of row r lands at
// position c ^ ((r >> 2) & 3) (the swizzle is applied to the per-lane SOURCE address, the DMA writes lane-linear), so that
// the ds_read_b128 of 8 rows hit 8 different bank groups without padding.  Chunks past D or G come from the zero page.  A
// fragment is 8 consecutive k per lane, split in registers: 44 VALU instructions next to the 12 MFMAs that consume it.
// LDS: 2 x 12 KB (A) + 3 x 8 KB (B) = 48 KB at MT = 2 -> three workgroups per CU; 3 x 6 + 24 = 42 KB at MT = 1.
struct F32RowsB {
    static constexpr int WAVE_PIECES = 2;
    static constexpr int STAGE_BYTES = RK_BN * 16 * sizeof(float);
    static constexpr bool SPLITS = true;
    struct Frag {
        f32x4 v0, v1;
    };
    const float* gal;
    const float* zeros;
    int D;
    const float* row[2];
    int k[2], off[2][2];
    bool ok[2];
    __device__ __forceinline__ void init(i64 n0, i64 G, int, int swave, int lane, int wn) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (swave * 2 + i) * 16 + (lane >> 2);
            ok[i] = n0 + r < G;
            row[i] = gal + (ok[i] ? (n0 + r) * D : 0);
            k[i] = ((lane & 3) ^ ((r >> 2) & 3)) * 4;
        }
        // fragment reads: row r = wn * 64 + j * 32 + lane % 32, chunks 2 * (lane >> 5) and + 1 at their swizzled positions
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = wn * 64 + j * 32 + (lane & 31), sw = (r >> 2) & 3, c0 = (lane >> 5) * 2;
            off[j][0] = r * 16 + ((c0 ^ sw) << 2);
            off[j][1] = r * 16 + (((c0 + 1) ^ sw) << 2);
        }
    }
    __device__ __forceinline__ void dma(char* Bs, int stage, int t, int swave) const {
        const int k0 = t * 16;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool in = ok[i] && k0 + k[i] < D;                    // D % 4 == 0: a chunk is inside or outside
            glds16(reinterpret_cast<const bf16_t*>(in ? row[i] + k0 + k[i] : zeros),
                   reinterpret_cast<bf16_t*>(Bs + stage * STAGE_BYTES + (swave * 2 + i) * 1024));
        }
    }
    __device__ __forceinline__ Frag read(const char* Bs, int stage, int j) const {
        const float* b = reinterpret_cast<const float*>(Bs + stage * STAGE_BYTES);
        return {*reinterpret_cast<const f32x4*>(b + off[j][0]), *reinterpret_cast<const f32x4*>(b + off[j][1])};
    }
    static __device__ __forceinline__ Planes3 planes(const Frag& f) {
        u32x4 h, m, l;
        split3(f.v0, f.v1, h, m, l);
        return {__builtin_bit_cast(bf16x8, h), __builtin_bit_cast(bf16x8, m), __builtin_bit_cast(bf16x8, l)};
    }
};

// A PREPARED gallery (mi355_gallery_prepare): the three bf16 planes of its normalised rows in the fragment order of
// k_split_queries ([row block of 32][k step][h, m, l][64 lanes][8], 6 B per element instead of 4), so B arrives as ready MFMA
// fragments like A: no split in the loop (round 2's PMC: matrix pipe 57 % busy + VALU 45 % busy, the 88 VALU instructions per
// fragment split did not co-issue with the MFMAs).  12 pieces per k-step, wave w moves pieces w, w + 4, w + 8; k-steps past
// the end re-read the last one.  LDS: 2 x 12 KB (A) + 3 x 12 KB (B) = 60 KB at MT = 2 (two workgroups per CU).
struct PlanesB {
    static constexpr int WAVE_PIECES = 3;
    static constexpr int STAGE_BYTES = (RK_BN / 32) * 3 * 1024;
    static constexpr bool SPLITS = false;
    typedef Planes3 Frag;
    const bf16_t* gs;
    const bf16_t* piece[3];
    int n_steps, frag0;
    __device__ __forceinline__ void init(i64 n0, i64, int steps, int swave, int lane, int wn) {
        n_steps = steps;
        frag0 = (wn * 2 * 3) * 512 + lane * 8;
        const bf16_t* src = gs + (size_t)(n0 / 32) * n_steps * 3 * 512 + lane * 8;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int p = swave + 4 * i;
            piece[i] = src + ((size_t)((p / 3) * n_steps) * 3 + p % 3) * 512;
        }
    }
    __device__ __forceinline__ void dma(char* Bs, int stage, int t, int swave) const {
        const int tt = t < n_steps ? t : n_steps - 1;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            glds16(piece[i] + (size_t)tt * 3 * 512, reinterpret_cast<bf16_t*>(Bs + stage * STAGE_BYTES + (swave + 4 * i) * 1024));
    }
    __device__ __forceinline__ Frag read(const char* Bs, int stage, int j) const {
        const bf16_t* b = reinterpret_cast<const bf16_t*>(Bs + stage * STAGE_BYTES) + frag0 + j * 3 * 512;
        return {*reinterpret_cast<const bf16x8*>(b), *reinterpret_cast<const bf16x8*>(b + 512),
                *reinterpret_cast<const bf16x8*>(b + 1024)};
    }
    static __device__ __forceinline__ Planes3 planes(const Frag& f) { return f; }
};

// One tile of either: scores are bit-identical between the two B operands, since the planes are the same values (split3 of
// the same fp32 rows) and the six products below are the only ones there are.
template <int MT, class B, class Epi>
__device__ __forceinline__ void cos_gemm_split_tile(const bf16_t* __restrict__ Qs, B bop, const float* __restrict__ ginv, int Q,
                                                    i64 G, int x0, int ntx, int n_steps, int xtiles, int ny, const Epi& epi) {
    constexpr int BM = 64 * MT;
    constexpr int A_PIECES = (BM / 32) * 3;           // 1 KB pieces per stage
    constexpr int A_STAGE = A_PIECES * 512;           // bf16 elements per stage
    constexpr int A_RING = SPLIT_A_RING<MT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    bf16_t* As = reinterpret_cast<bf16_t*>(smem);                       // [A_RING][BM/32][3][512]
    char* Bs = reinterpret_cast<char*>(As + A_RING * A_STAGE);          // [3][B::STAGE_BYTES]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by;
    rank_tile_of((int)blockIdx.x, xtiles, ny, bx, by);
    const i64 n0 = (i64)(bx + x0) * RK_BN;
    const int m0 = by * BM;
    // the wave index as a scalar: piece selection becomes scalar branches (a per-lane branch around a load makes hipcc
    // drain vmcnt)
    const int swave = __builtin_amdgcn_readfirstlane(wave);

    bop.init(n0, G, n_steps, swave, lane, wn);
    auto dma_b = [&](int stage, int t) { bop.dma(Bs, stage, t, swave); };
    // A: piece (row block rbl, plane p) of k-step t sits at Qs + (((m0/32 + rbl) * n_steps + t) * 3 + p) * 512.
    // 12 (MT = 2) or 6 (MT = 1) pieces per stage: wave w moves pieces w, w + 4, w + 8 / pieces w and (w < 2) w + 4.
    const bf16_t* a_src = Qs + (size_t)(m0 / 32) * n_steps * 3 * 512 + lane * 8;
    const bf16_t* a_piece[(A_PIECES + 3) / 4];
#pragma unroll
    for (int i = 0; i < (A_PIECES + 3) / 4; ++i) {
        const int piece = (swave + 4 * i) % A_PIECES;
        a_piece[i] = a_src + ((size_t)((piece / 3) * n_steps) * 3 + piece % 3) * 512;
    }
    auto dma_a = [&](int buf, int t) {
#pragma unroll
        for (int i = 0; i < (A_PIECES + 3) / 4; ++i) {
            const int piece = swave + 4 * i;
            if (A_PIECES % 4 == 0 || i < A_PIECES / 4 || swave < A_PIECES % 4)
                glds16(a_piece[i] + (size_t)t * 3 * 512, As + buf * A_STAGE + piece * 512);
        }
    };

    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    auto compute = [&](int abuf, int bstage) {
        const bf16_t* a = As + abuf * A_STAGE + (wm * MT * 3) * 512 + lane * 8;
        bf16x8 af[MT][3];
        typename B::Frag bf[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = bop.read(Bs, bstage, j);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int p = 0; p < 3; ++p) af[i][p] = *reinterpret_cast<const bf16x8*>(a + (i * 3 + p) * 512);
        // Per fragment j: six products for each of the MT row blocks, smallest terms first (the order is the same for every
        // (query, gallery row) pair wherever its tile lies and however B arrived).
        auto products = [&](int j, const Planes3& g) {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][2], g.h, acc[i][j], 0, 0, 0);   // l * h'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], g.l, acc[i][j], 0, 0, 0);   // h * l'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], g.m, acc[i][j], 0, 0, 0);   // m * m'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], g.h, acc[i][j], 0, 0, 0);   // m * h'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], g.m, acc[i][j], 0, 0, 0);   // h * m'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], g.h, acc[i][j], 0, 0, 0);   // h * h'
            }
        };
        const Planes3 g0 = B::planes(bf[0]), g1 = B::planes(bf[1]);
        products(0, g0);
        // The split of fragment 1 is issued in the gaps of fragment 0's MFMAs (an MFMA holds the vector issue for 8 of its 32
        // cycles): sched_group_barrier pins "1 MFMA, 4 VALU" groups.
        if constexpr (B::SPLITS) {
#pragma unroll
            for (int g = 0; g < 6 * MT; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);   // four VALU (of fragment 1's split)
            }
        }
        products(1, g1);
    };

    dma_ring<A_RING, A_PIECES, B::WAVE_PIECES>(n_steps, swave, dma_a, dma_b, compute);
    epi.tile(acc, smem, ginv, TileCtx{Q, G, ntx, n0, m0});
}
template <int MT, int FK>
__global__ __launch_bounds__(256, 3) void k_cos_gemm_split(const bf16_t* __restrict__ Qs, const float* __restrict__ Gal,
                                                           const float* __restrict__ ginv, int Q, i64 G, int D, int x0, int ntx,
                                                           int n_steps, const float* __restrict__ zeros, int xtiles, int ny,
                                                           PlainEpi<FK> epi) {
    cos_gemm_split_tile<MT>(Qs, F32RowsB{Gal, zeros, D}, ginv, Q, G, x0, ntx, n_steps, xtiles, ny, epi);
}
template <int MT, class Epi>
__global__ __launch_bounds__(256, 3) void k_cos_gemm_split_epi(const bf16_t* __restrict__ Qs, const float* __restrict__ Gal,
                                                               const float* __restrict__ ginv, int Q, i64 G, int D, int x0,
                                                               int ntx, int n_steps, const float* __restrict__ zeros, int xtiles,
                                                               int ny, Epi epi) {
    cos_gemm_split_tile<MT>(Qs, F32RowsB{Gal, zeros, D}, ginv, Q, G, x0, ntx, n_steps, xtiles, ny, epi);
}

template <int MT, int FK>
__global__ __launch_bounds__(256, 2) void k_cos_gemm_pre(const bf16_t* __restrict__ Qs, const bf16_t* __restrict__ Gs, int Q,
                                                         i64 G, int x0, int ntx, int n_steps, int xtiles, int ny,
                                                         SelectEpi<FK, false> epi) {
    cos_gemm_split_tile<MT>(Qs, PlanesB{Gs}, nullptr, Q, G, x0, ntx, n_steps, xtiles, ny, epi);
}

// =====================================================================================
// few queries (Q <= 4, the reference's own per-query call shape cos(q[None], G), train/train.py:250): a GEMM tile
// would be 98 % padding; this is a GEMV, bound by streaming the gallery once (4*D bytes per row).  One wave per
// gallery row (6 KB contiguous for D = 1536), the normalised queries sit in LDS, two rows in flight per wave.
// =====================================================================================
template <int NQ>
__global__ __launch_bounds__(256) void k_cos_gemv(const float* __restrict__ Qn, const float* __restrict__ Gal,
                                                  const float* __restrict__ ginv, float* __restrict__ S, i64 G, int D,
                                                  int vec) {
    extern __shared__ __attribute__((aligned(16))) float qs[];   // [NQ][D]
    for (int i = threadIdx.x; i < NQ * D; i += 256) qs[i] = Qn[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const i64 wave_id = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 g = wave_id; g < G; g += nwaves) {
        const float* row = Gal + g * D;
        float acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
        if (vec) {
            const f32x4* r4 = reinterpret_cast<const f32x4*>(row);
#pragma unroll 2
            for (int i = lane; i < D / 4; i += 64) {
                const f32x4 v = r4[i];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const f32x4 u = *reinterpret_cast<const f32x4*>(&qs[q * D + i * 4]);
                    acc[q] += v.x * u.x + v.y * u.y + v.z * u.z + v.w * u.w;
                }
            }
        } else {
            for (int i = lane; i < D; i += 64) {
                const float v = row[i];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += v * qs[q * D + i];
            }
        }
        const float gs = ginv ? ginv[g] : 1.0f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float t = wave_sum(acc[q]);
            if (lane == 0) S[(i64)q * G + g] = t * gs;
        }
    }
}

// ---- small k (<= 8): per-thread sorted list in registers, then k rounds of block arg-max.
// grid = (nchunk, Q).  Input row q: vals[q*in_stride + j], j in [0,rowlen); implicit index j (+offset)
// when idxs == nullptr.  Output: out[(q*nchunk + chunk)*k + r].
// idxs32 (optional): int32 LOCAL indices from the fused GEMM epilogue (IDX32_PAD = missing); idx_offset is added to them.
template <int K>
__global__ __launch_bounds__(256) void k_topk_small(const float* __restrict__ vals, const i64* __restrict__ idxs,
                                                    const int* __restrict__ idxs32,
                                                    i64 rowlen, i64 in_stride, i64 chunk_len, int k,
                                                    i64 idx_offset, float* __restrict__ ov, i64* __restrict__ oi) {
    constexpr bool FILT = false;
    const RankFilter flt{};
#include "rank_topk_small.inc"
}
template <int K>
__global__ __launch_bounds__(256) void k_topk_small_filt(const float* __restrict__ vals, i64 rowlen, i64 in_stride,
                                                         i64 chunk_len, int k, i64 idx_offset, float* __restrict__ ov,
                                                         i64* __restrict__ oi, RankFilter flt) {
    constexpr bool FILT = true;
    const i64* const idxs = nullptr;
    const int* const idxs32 = nullptr;
#include "rank_topk_small.inc"
}

// ---- any k <= 1024: bitonic sort of a 2048-element chunk in LDS, keep the first k.
constexpr int BT_N = 2048;
__global__ __launch_bounds__(256) void k_topk_bitonic(const float* __restrict__ vals, const i64* __restrict__ idxs,
                                                      i64 rowlen, i64 in_stride, int k, i64 idx_offset,
                                                      float* __restrict__ ov, i64* __restrict__ oi) {
    constexpr bool FILT = false;
    const RankFilter flt{};
#include "rank_topk_bitonic.inc"
}
__global__ __launch_bounds__(256) void k_topk_bitonic_filt(const float* __restrict__ vals, i64 rowlen, i64 in_stride, int k,
                                                           i64 idx_offset, float* __restrict__ ov, i64* __restrict__ oi,
                                                           RankFilter flt) {
    constexpr bool FILT = true;
    const i64* const idxs = nullptr;
#include "rank_topk_bitonic.inc"
}

// Indices outside [lo, hi) -> (-inf, -1): the pads a filtered search leaves when fewer than k rows are eligible
__global__ __launch_bounds__(256) void k_clear_pads(float* __restrict__ v, i64* __restrict__ ix, i64 n, i64 lo, i64 hi) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t < n && (ix[t] < lo || ix[t] >= hi)) { v[t] = NEG_INF; ix[t] = -1; }
}

// =====================================================================================
// small ops
// =====================================================================================
__global__ __launch_bounds__(256) void k_pair_cosine(const float* __restrict__ a, const float* __restrict__ b,
                                                     i64 rows, int dim, float eps, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = a + row * dim;
    const float* y = b + row * dim;
    float xx = 0.f, yy = 0.f, xy = 0.f;
    for (int i = lane; i < dim; i += 64) {
        const float u = x[i], w = y[i];
        xx += u * u; yy += w * w; xy += u * w;
    }
    xx = wave_sum(xx); yy = wave_sum(yy); xy = wave_sum(xy);
    if (lane == 0) out[row] = xy / (fmaxf(sqrtf(xx), eps) * fmaxf(sqrtf(yy), eps));
}

// One block of 16 waves; wave w owns rows w, w+16, ... and adds them in that order, then thread 0
// adds the 16 wave partials in wave order: the result is a fixed function of the inputs.
__global__ __launch_bounds__(1024) void k_contrastive(const float* __restrict__ f1, const float* __restrict__ f2,
                                                      i64 rows, int dim, float label, float margin, int mean,
                                                      float* __restrict__ out, float* __restrict__ per_row) {
    __shared__ float part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc = 0.f;
    for (i64 r = wave; r < rows; r += 16) {
        const float* x = f1 + r * dim;
        const float* y = f2 + r * dim;
        float d = 0.f;
        for (int i = lane; i < dim; i += 64) {
            const float t = y[i] - x[i];
            d += t * t;
        }
        d = wave_sum(d);
        const float h = fmaxf(margin - sqrtf(d + 1e-9f), 0.f);
        const float l = 0.5f * (label * d + (1.0f - label) * h * h);
        if (per_row && lane == 0) per_row[r] = l;
        acc += l;
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int w = 0; w < 16; ++w) s += part[w];
        out[0] = mean ? s / (float)rows : s;
    }
}

// torch.nn.CosineEmbeddingLoss (ATen cosine_embedding_loss): cos = xy / sqrt((xx + 1e-12)(yy + 1e-12));
// target +1 -> 1 - cos, target -1 -> max(0, cos - margin); mean (or sum) over rows in a fixed order.
__global__ __launch_bounds__(1024) void k_cos_embedding_loss(const float* __restrict__ f1, const float* __restrict__ f2,
                                                             i64 rows, int dim, float target, float margin, int mean,
                                                             float* __restrict__ out) {
    __shared__ float part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc = 0.f;
    for (i64 r = wave; r < rows; r += 16) {
        const float* x = f1 + r * dim;
        const float* y = f2 + r * dim;
        float xx = 0.f, yy = 0.f, xy = 0.f;
        for (int i = lane; i < dim; i += 64) {
            const float u = x[i], v = y[i];
            xx += u * u; yy += v * v; xy += u * v;
        }
        xx = wave_sum(xx); yy = wave_sum(yy); xy = wave_sum(xy);
        const float c = xy / sqrtf((xx + 1e-12f) * (yy + 1e-12f));
        acc += target > 0.f ? 1.0f - c : fmaxf(c - margin, 0.f);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += part[w];
        out[0] = mean ? t / (float)rows : t;
    }
}

// An index outside [0, G) (a pad entry of a list with fewer than k real candidates) counts as a miss.
// packed candidate lists of the sharded search (see mi355_pack_candidates / mi355_merge_packed_topk)
__global__ __launch_bounds__(256) void k_pack_candidates(const float* __restrict__ val, const i64* __restrict__ idx, i64 Q,
                                                         int kk, int k, int* __restrict__ packed) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t >= Q * k) return;
    const i64 q = t / k;
    const int j = (int)(t - q * k);
    int2 o;
    if (j < kk) { o.x = __float_as_int(val[q * kk + j]); o.y = (int)idx[q * kk + j]; }
    else { o.x = __float_as_int(NEG_INF); o.y = -1; }
    reinterpret_cast<int2*>(packed)[t] = o;
}

constexpr i64 PACKED_PAD_IDX = NO_CAND_IDX;     // "no candidate" (the selection skips it): a slot no shard filled
__global__ __launch_bounds__(256) void k_unpack_candidates(const int* __restrict__ packed, const i64* __restrict__ offsets,
                                                           int world, i64 Q, int k, float* __restrict__ cv, i64* __restrict__ ci) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;      // output slot: query q, candidate (r, j) = r * k + j
    const i64 per = (i64)world * k;
    if (t >= Q * per) return;
    const i64 q = t / per;
    const int c = (int)(t - q * per), r = c / k, j = c - r * k;
    const int2 p = reinterpret_cast<const int2*>(packed)[((i64)r * Q + q) * k + j];
    cv[t] = __int_as_float(p.x);
    ci[t] = p.y >= 0 ? (i64)p.y + offsets[r] : PACKED_PAD_IDX;
}

__global__ void k_hit_counts(const i64* __restrict__ idx, i64 Q, int k, const i64* __restrict__ qcls,
                             const i64* __restrict__ gcls, i64 G, i64* __restrict__ counts) {
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    int h1 = 0, h3 = 0;
    if (q < Q) {
        const i64 c = qcls[q];
        for (int j = 0; j < min(k, 3); ++j) {
            const i64 g = idx[q * k + j];
            const int hit = (g >= 0 && g < G) ? (gcls[g] == c) : 0;
            if (j == 0) h1 = hit;
            h3 |= hit;
        }
    }
    // integer atomics: order-independent
    const unsigned long long m1 = __ballot(h1), m3 = __ballot(h3);
    if ((threadIdx.x & 63) == 0) {
        if (m1) atomicAdd((unsigned long long*)&counts[0], (unsigned long long)__popcll(m1));
        if (m3) atomicAdd((unsigned long long*)&counts[1], (unsigned long long)__popcll(m3));
    }
}

__global__ void k_distinct_topn(const i64* __restrict__ idx, const float* __restrict__ val, i64 Q, int k,
                                const i64* __restrict__ gcls, i64 G, int n, i64* __restrict__ ocls,
                                i64* __restrict__ oidx, float* __restrict__ oval) {
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    i64 seen[8];
    int ns = 0;
    for (int j = 0; j < n; ++j) { ocls[q * n + j] = -1; oidx[q * n + j] = -1; oval[q * n + j] = NAN; }
    for (int j = 0; j < k && ns < n; ++j) {
        const i64 g = idx[q * k + j];
        if (g < 0 || g >= G) continue;          // pad entry: not a candidate
        const i64 c = gcls[g];
        bool dup = false;
#pragma unroll
        for (int s = 0; s < 8; ++s) dup |= (s < ns && seen[s] == c);
        if (!dup) {
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (s == ns) seen[s] = c;
            ocls[q * n + ns] = c; oidx[q * n + ns] = g; oval[q * n + ns] = val[q * k + j];
            ++ns;
        }
    }
}

// Relevance metrics of one ranked list per wave (mi355_retrieval_metrics): rank i is relevant when its row has the query's
// class.  The running count of relevant ranks comes from a ballot per 64 ranks; the MAP@R terms are summed per lane in rank
// order and then across the wave in a fixed tree, so the result is a fixed function of the inputs.
__global__ __launch_bounds__(256) void k_retrieval_metrics(const i64* __restrict__ idx, i64 Q, int k, const i64* __restrict__ qcls,
                                                           const i64* __restrict__ gcls, i64 G, const i64* __restrict__ R,
                                                           double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const i64 q = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const i64 c = qcls[q], Rq = R[q];
    int first = k, run = 0, hits = 0;
    double ap = 0.0;
    for (int i0 = 0; i0 < k; i0 += 64) {
        const int i = i0 + lane;
        bool rel = false;
        if (i < k) {
            const i64 g = idx[q * k + i];
            rel = g >= 0 && g < G && gcls[g] == c;
        }
        const unsigned long long m = __ballot(rel);
        if (first == k && m) first = i0 + __ffsll((long long)m) - 1;
        const int cum = run + __popcll(m & ((1ull << lane) - 1)) + (rel ? 1 : 0);     // relevant ranks 0 .. i
        if (rel && i < Rq) ap += (double)cum / (double)(i + 1);
        hits += __popcll(__ballot(rel && i < Rq));
        run += __popcll(m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ap += __shfl_xor(ap, o, 64);
    if (lane == 0) {
        double* o = out + q * 3;
        o[0] = first;
        o[1] = Rq > 0 ? (double)hits / (double)Rq : 0.0;
        o[2] = Rq > 0 ? ap / (double)Rq : 0.0;
    }
}

// =====================================================================================
// host drivers
// =====================================================================================
constexpr i64 SMALL_CHUNK = 8192;

struct TopkPlan {
    bool small;
    i64 nchunk1;        // level-1 chunks per row
    size_t cand_elems;  // elements per ping/pong candidate buffer (per query row) * Q
};

static i64 level1_chunks(i64 G, int k) { return k <= SMALL_K ? cdiv(G, SMALL_CHUNK) : cdiv(G, BT_N); }

size_t topk_ws_bytes(i64 Q, i64 G, int k) {
    const i64 per_row = level1_chunks(G, k) * k;
    // two ping-pong buffers of (val f32 + idx i64)
    return 2 * align_up((size_t)Q * per_row * (sizeof(float) + sizeof(i64)), 256) + 256;
}

// filt (first level of a filtered search, implicit indices): k_topk_small_filt
template <int K>
static void launch_small(const float* v, const i64* ix, const int* ix32, i64 rowlen, i64 in_stride, i64 chunk_len, int k,
                         i64 off, float* ov, i64* oi, i64 nchunk, i64 Q, hipStream_t st, const RankFilter* filt) {
    if (filt)
        hipLaunchKernelGGL((k_topk_small_filt<K>), dim3((unsigned)nchunk, (unsigned)Q), dim3(256), 0, st, v, rowlen, in_stride,
                           chunk_len, k, off, ov, oi, *filt);
    else
        hipLaunchKernelGGL((k_topk_small<K>), dim3((unsigned)nchunk, (unsigned)Q), dim3(256), 0, st, v, ix, ix32, rowlen,
                           in_stride, chunk_len, k, off, ov, oi);
}
static void dispatch_small(const float* v, const i64* ix, const int* ix32, i64 rowlen, i64 in_stride, i64 chunk_len, int k,
                           i64 off, float* ov, i64* oi, i64 nchunk, i64 Q, hipStream_t st, const RankFilter* filt) {
    if (k <= 1) launch_small<1>(v, ix, ix32, rowlen, in_stride, chunk_len, k, off, ov, oi, nchunk, Q, st, filt);
    else if (k <= 2) launch_small<2>(v, ix, ix32, rowlen, in_stride, chunk_len, k, off, ov, oi, nchunk, Q, st, filt);
    else if (k <= 4) launch_small<4>(v, ix, ix32, rowlen, in_stride, chunk_len, k, off, ov, oi, nchunk, Q, st, filt);
    else launch_small<8>(v, ix, ix32, rowlen, in_stride, chunk_len, k, off, ov, oi, nchunk, Q, st, filt);
}

static thread_local int g_rank_path = 0;
void set_rank_path(int path) { g_rank_path = path; }

RankFilter filter_from(const RankFilter& f, i64 q0) {
    RankFilter r = f;
    if (r.qlab) r.qlab += q0;
    if (r.excl) r.excl += q0;
    return r;
}

int make_filter(const mi355_rank_filter* f, i64 idx_offset, const char* who, RankFilter* out) {
    MI355_REQUIRE(f, "%s: null filter (use the unfiltered entry)", who);
    MI355_REQUIRE(f->label_mode == MI355_LABEL_ANY || f->label_mode == MI355_LABEL_SAME || f->label_mode == MI355_LABEL_DIFFERENT,
                  "%s: unknown label_mode %d", who, f->label_mode);
    MI355_REQUIRE(f->label_mode == MI355_LABEL_ANY || (f->query_labels && f->gallery_labels),
                  "%s: label_mode %d needs query_labels and gallery_labels (null pointer)", who, f->label_mode);
    out->qlab = f->label_mode != MI355_LABEL_ANY ? (const i64*)f->query_labels : nullptr;
    out->glab = f->label_mode != MI355_LABEL_ANY ? (const i64*)f->gallery_labels : nullptr;
    out->excl = (const i64*)f->exclude;
    out->idx_offset = idx_offset;
    out->mode = f->label_mode;
    return OK;
}

// Select top-k of each row of vals[Q][rowlen] (implicit or explicit indices) into out_val/out_idx [Q][k].
// idxs32 (with idxs == nullptr): int32 local candidate indices of the fused GEMM epilogue, k <= SMALL_K only.
int topk_select(const float* vals, const i64* idxs, i64 Q, i64 rowlen, i64 in_stride, int k, i64 idx_offset,
                float* out_val, i64* out_idx, void* ws, size_t ws_bytes, hipStream_t st, const int* idxs32,
                const RankFilter* filt) {
    MI355_REQUIRE(k >= 1 && k <= LARGE_K, "top-k: k=%d outside [1,%d]", k, LARGE_K);
    MI355_REQUIRE(k <= rowlen, "top-k: k=%d exceeds row length %lld", k, (long long)rowlen);
    MI355_REQUIRE(!idxs32 || k <= SMALL_K, "top-k: int32 candidate lists need k <= %d", SMALL_K);
    MI355_REQUIRE(Q >= 1 && Q <= 65535 * 16, "top-k: Q=%lld out of range", (long long)Q);
    MI355_REQUIRE(ws_bytes >= topk_ws_bytes(Q, rowlen, k), "top-k: workspace %zu < %zu bytes", ws_bytes,
                  topk_ws_bytes(Q, rowlen, k));
    const i64 per_row_max = level1_chunks(rowlen, k) * k;
    const size_t half = align_up((size_t)Q * per_row_max * (sizeof(float) + sizeof(i64)), 256);
    char* base = align256(ws);
    float* cv[2];
    i64* ci[2];
    for (int b = 0; b < 2; ++b) {
        ci[b] = (i64*)(base + b * half);
        cv[b] = (float*)(base + b * half + (size_t)Q * per_row_max * sizeof(i64));
    }
    // grid.y limit: split Q into slabs of 65535 rows
    for (i64 qs = 0; qs < Q; qs += 65535) {
        const i64 qn = (Q - qs < 65535) ? Q - qs : 65535;
        const float* v = vals + qs * in_stride;
        const i64* ix = idxs ? idxs + qs * in_stride : nullptr;
        const int* ix32 = idxs32 ? idxs32 + qs * in_stride : nullptr;
        i64 len = rowlen, stride = in_stride;
        i64 off = idx_offset;
        int cur = 0;
        // the filter applies where candidates carry implicit indices (the first level over a score slab); the fused
        // epilogue applied it already, later levels carry its pads
        RankFilter fs{};
        if (filt) fs = filter_from(*filt, qs);
        const RankFilter* f1 = (filt && !ix && !ix32) ? &fs : nullptr;
        while (true) {
            const bool small = (k <= SMALL_K);
            const i64 chunk = small ? SMALL_CHUNK : BT_N;
            const i64 nchunk = cdiv(len, chunk);
            const bool last = (nchunk == 1);
            float* ovp = last ? out_val + qs * k : cv[cur];
            i64* oip = last ? out_idx + qs * k : ci[cur];
            if (small) dispatch_small(v, ix, ix32, len, stride, chunk, k, off, ovp, oip, nchunk, qn, st, f1);
            else if (f1) hipLaunchKernelGGL(k_topk_bitonic_filt, dim3((unsigned)nchunk, (unsigned)qn), dim3(256), 0, st, v, len,
                                            stride, k, off, ovp, oip, *f1);
            else hipLaunchKernelGGL(k_topk_bitonic, dim3((unsigned)nchunk, (unsigned)qn), dim3(256), 0, st, v, ix,
                                    len, stride, k, off, ovp, oip);
            MI355_LAUNCH_CHECK();
            if (last) break;
            v = cv[cur]; ix = ci[cur]; ix32 = nullptr; f1 = nullptr;
            len = nchunk * k; stride = len; off = 0;
            cur ^= 1;
        }
    }
    if (filt) {
        hipLaunchKernelGGL(k_clear_pads, dim3((unsigned)cdiv(Q * k, 256)), dim3(256), 0, st, out_val, out_idx, Q * k, (i64)LLONG_MIN,
                           IDX_PAD);
        MI355_LAUNCH_CHECK();
    }
    return OK;
}

bool fused_select(i64 Q, i64 G, int k) { return k >= 1 && k <= SMALL_K && Q > 4 && G < ((i64)1 << 31) - RK_BN; }

i64 query_block(i64 Q, i64 G, int k) {
    if (fused_select(Q, G, k)) {
        // no score slab: candidates are cdiv(G,128) * k * 8 B per query; keep them <= 32 MiB per block of queries (a second
        // block costs one more pass over the gallery, which a GEMM of >= 1000 queries hides)
        i64 qb = ((i64)1 << 25) / (cdiv(G, RK_BN) * (i64)k * 8);
        qb = qb / 128 * 128;
        if (qb < 128) qb = 128;
        return qb < Q ? qb : Q;
    }
    // keep the score slab S[qb][G] around <= 1 GiB, in multiples of 256 queries
    i64 qb = ((i64)1 << 28) / (G > 0 ? G : 1);
    qb = qb / 256 * 256;
    if (qb < 256) qb = 256;
    return qb < Q ? qb : Q;
}

// split planes of rows (k_split_queries): whole 128-row tiles, 16-deep k steps, three planes, then the zero page
static size_t split_queries_bytes(i64 Q, int D) { return (size_t)cdiv(Q, 128) * 4 * cdiv(D, 16) * 3 * 1024 + 256; }
// rows [0, n) of x -> their split planes (k_split_queries)
static int split_rows(const float* x, i64 n, int D, bf16_t* planes, hipStream_t st) {
    const int n_steps = cdiv(D, 16);
    const i64 n_frag = (i64)cdiv(n, 128) * 4 * n_steps;
    hipLaunchKernelGGL(k_split_queries, dim3((unsigned)cdiv(n_frag, 4)), dim3(256), 0, st, x, planes, (int)n, D, n_steps, (int)n_frag);
    MI355_LAUNCH_CHECK();
    return OK;
}

RankWs carve(void* ws, i64 Q, i64 G, int D, int k, size_t (*planes_bytes)(i64, int), bool need_ginv, bool need_S) {
    RankWs r{};
    const bool fused = need_S && fused_select(Q, G, k);
    const i64 qb = query_block(Q, G, need_S ? k : 0);
    WsCarver c(ws);
    r.qn = (float*)c.take((size_t)Q * D * sizeof(float));
    const i64 q_split = need_S ? qb : (Q < 256 * 64 ? Q : 256 * 64);      // queries of one cos_gemm call
    r.qs = c.take(planes_bytes ? planes_bytes(q_split, D) : 0);
    r.ginv = (float*)c.take(need_ginv ? (size_t)G * sizeof(float) : 0);
    if (fused) {
        const size_t ncand = (size_t)qb * cdiv(G, RK_BN) * k;
        r.cand_val = (float*)c.take(ncand * sizeof(float));
        r.cand_idx = (int*)c.take(ncand * sizeof(int));
        r.topk_bytes = topk_ws_bytes(qb, cdiv(G, RK_BN) * (i64)k, k);
    } else {
        r.S = (float*)c.take(need_S ? (size_t)qb * G * sizeof(float) : 0);
        r.topk_bytes = k > 0 ? topk_ws_bytes(qb, G, k) : 0;
    }
    r.topk = c.take(r.topk_bytes);
    r.total = c.total();
    return r;
}

// resident workgroups per CU x CUs of the current device for one kernel instantiation (cached per device by the caller)
int kernel_slots(const void* fn, size_t lds, int* cache, int* slots_out) {
    int dev = 0;
    MI355_CHECK_HIP(hipGetDevice(&dev));
    MI355_REQUIRE(dev >= 0 && dev < MI355_MAX_DEVICES, "rank: device ordinal %d out of range", dev);
    if (!cache[dev]) {
        MI355_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int per_cu = 0, cus = 0;
        MI355_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds));
        MI355_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        cache[dev] = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
    }
    *slots_out = cache[dev];
    return OK;
}

int whole_round_tiles(int ntx, int ny, int slots) {
    if ((long)ntx * ny > slots && ((long)ntx * ny) % slots != 0) return (int)(((long)ntx * ny / slots) * slots / ny);
    return ntx;
}

// Test override of the slots (0: the device's own) and the last cut, per thread like the rank path
static thread_local int g_round_slots = 0;
static thread_local int g_last_tiles[5] = {0, 0, 0, 0, 0};
int round_slots(int device_slots) { return g_round_slots > 0 ? g_round_slots : device_slots; }
void set_last_tiles(int slots, int ny, int main_tiles, int tail_tiles, int tail_ny) {
    g_last_tiles[0] = slots; g_last_tiles[1] = ny; g_last_tiles[2] = main_tiles; g_last_tiles[3] = tail_tiles;
    g_last_tiles[4] = tail_ny;
}

// ---- the tiled GEMM families of this file (launch_tiles, rank_common.h)
// Exact fp32 loop (qry: the normalised fp32 rows).  Tile choice, measured on MI355X (tools/bench_rank.py, D = 1536): it
// plateaus at 95-110 TFLOP/s for every tile shape, so what differs is the partial last round of tiles.  128-query tiles with
// BK = 16 keep two workgroups on a CU (41 KB of staging, 68 KB with the fused selection's score tile): a lone workgroup in
// the last round runs at full speed, which halves the wave-quantisation loss (Q = 256, G = 100k: 0.83 ms, against 0.95 ms
// with 256 x 128 tiles, one per CU).  64-query tiles use BK = 32.
template <bool VEC>
struct F32Gemm {
    template <int MT> static constexpr int BK = MT == 2 ? 16 : 32;
    template <int MT> static constexpr size_t stage_bytes() { return (size_t)2 * (64 * MT + RK_BN) * (BK<MT> + 4) * sizeof(float); }
    template <int MT, class Epi> static constexpr auto kernel() {
        if constexpr (plain_fk<Epi> >= 0) return &k_cos_gemm<MT, BK<MT>, VEC, plain_fk<Epi>>;
        else return &k_cos_gemm_epi<MT, BK<MT>, VEC, Epi>;
    }
    template <int MT, class Epi>
    static void launch(dim3 grid, size_t lds, hipStream_t st, const TileArgs& a, const Epi& epi, int x0, int ntx, int xtiles, int ny) {
        hipLaunchKernelGGL((kernel<MT, Epi>()), grid, dim3(256), lds, st, (const float*)a.qry, (const float*)a.gal, a.ginv, a.Q, a.G,
                           a.D, x0, ntx, xtiles, ny, epi);
    }
};

// Split-bf16 loop (qry: the split planes of the queries, split_rows; gal: fp32 rows with D % 4 == 0)
struct SplitGemm {
    template <int MT> static constexpr size_t stage_bytes() { return SPLIT_A_BYTES<MT> + 3 * F32RowsB::STAGE_BYTES; }
    template <int MT, class Epi> static constexpr auto kernel() {
        if constexpr (plain_fk<Epi> >= 0) return &k_cos_gemm_split<MT, plain_fk<Epi>>;
        else return &k_cos_gemm_split_epi<MT, Epi>;
    }
    template <int MT, class Epi>
    static void launch(dim3 grid, size_t lds, hipStream_t st, const TileArgs& a, const Epi& epi, int x0, int ntx, int xtiles, int ny) {
        const bf16_t* qs = (const bf16_t*)a.qry;
        const int n_steps = cdiv(a.D, 16);
        const float* zeros = reinterpret_cast<const float*>(qs + (size_t)cdiv(a.Q, 128) * 4 * n_steps * 3 * 512);
        hipLaunchKernelGGL((kernel<MT, Epi>()), grid, dim3(256), lds, st, qs, (const float*)a.gal, a.ginv, a.Q, a.G, a.D, x0, ntx,
                           n_steps, zeros, xtiles, ny, epi);
    }
};

// Prepared gallery (qry: the split planes of the queries; gal: the gallery's planes): the unfiltered fused selection only
struct PreparedGemm {
    template <int MT> static constexpr size_t stage_bytes() { return SPLIT_A_BYTES<MT> + 3 * PlanesB::STAGE_BYTES; }
    template <int MT, class Epi> static constexpr auto kernel() {
        static_assert(plain_fk<Epi> > 0, "the prepared gallery has fused unfiltered kernels only");
        return &k_cos_gemm_pre<MT, plain_fk<Epi>>;
    }
    template <int MT, class Epi>
    static void launch(dim3 grid, size_t lds, hipStream_t st, const TileArgs& a, const Epi& epi, int x0, int ntx, int xtiles, int ny) {
        hipLaunchKernelGGL((kernel<MT, Epi>()), grid, dim3(256), lds, st, (const bf16_t*)a.qry, (const bf16_t*)a.gal, a.Q, a.G, x0,
                           ntx, cdiv(a.D, 16), xtiles, ny, epi);
    }
};

// MI355_RANK_EXACT_F32=1 keeps the GEMM on v_mfma_f32_32x32x2_f32 (a bit-for-bit fmaf chain, 2.7x the matrix-pipe time);
// the default is the three-way bf16 split with six products (fp32-equivalent, see split3).
static bool rank_exact_f32() {
    const char* e = getenv("MI355_RANK_EXACT_F32");
    return e && e[0] && e[0] != '0';
}

// One GEMM call over fp32 rows: the normalised queries qn [Q][D] against gal with epilogue epi.
// qs: scratch for the split planes of these Q queries (split_queries_bytes(Q, D)); may be null for Q <= 4.
// Only the score slab has a GEMV (Q <= 4); every other epilogue runs on the tiles for any Q (the GEMV's bits differ).
template <class Epi>
static int cos_gemm(const float* qn, bf16_t* qs, const float* gal, const float* ginv, i64 Q, i64 G, int D, const Epi& epi,
                    hipStream_t st) {
    const bool vec = vec_ok(qn, D) && vec_ok(gal, D);
    constexpr int fused_bit = is_select<Epi> ? MI355_RANK_PATH_FUSED : 0;
    if constexpr (std::is_same_v<Epi, SlabEpi>) {
        if (Q <= 4 && (size_t)Q * D * sizeof(float) <= 60 * 1024) {
            set_rank_path(MI355_RANK_PATH_GEMV);
            const size_t lds = (size_t)Q * D * sizeof(float);
            const unsigned blocks = (unsigned)(cdiv(G, 4) < 4096 ? cdiv(G, 4) : 4096);
#define GEMV_LAUNCH(NQ) hipLaunchKernelGGL((k_cos_gemv<NQ>), dim3(blocks), dim3(256), lds, st, qn, gal, ginv, epi.S, G, D, (int)vec)
            if (Q == 1) GEMV_LAUNCH(1); else if (Q == 2) GEMV_LAUNCH(2); else if (Q == 3) GEMV_LAUNCH(3); else GEMV_LAUNCH(4);
#undef GEMV_LAUNCH
            MI355_LAUNCH_CHECK();
            return OK;
        }
    }
    TileArgs a{qn, gal, ginv, (int)Q, G, D};
    if (qs && vec_ok(gal, D) && !rank_exact_f32()) {
        if (int e = split_rows(qn, Q, D, qs, st)) return e;
        set_rank_path(MI355_RANK_PATH_SPLIT | fused_bit);
        a.qry = qs;
        return cos_gemm_tiles<SplitGemm>(a, epi, st);
    }
    set_rank_path(MI355_RANK_PATH_EXACT_F32 | fused_bit);
    return vec ? cos_gemm_tiles<F32Gemm<true>>(a, epi, st) : cos_gemm_tiles<F32Gemm<false>>(a, epi, st);
}

int normalize_search(const float* queries, i64 Q, const float* gallery, i64 G, int dim, float eps, const RankWs& w,
                     hipStream_t st) {
    const int vq = vec_ok(queries, dim) && vec_ok(w.qn, dim);
    RoctxRange range("rank/normalize");
    hipLaunchKernelGGL((k_row_norm<true>), dim3((unsigned)cdiv(Q, 4)), dim3(256), 0, st, queries, w.qn, (float*)nullptr, (i64)Q,
                       dim, eps, vq);
    MI355_LAUNCH_CHECK();
    if (gallery) {
        hipLaunchKernelGGL((k_row_norm<false>), dim3((unsigned)cdiv(G, 4)), dim3(256), 0, st, gallery, (float*)nullptr, w.ginv,
                           (i64)G, dim, eps, vec_ok(gallery, dim));
        MI355_LAUNCH_CHECK();
    }
    return OK;
}

static int check_rank_args(const float* queries, i64 Q, const float* gallery, i64 G, int dim) {
    MI355_REQUIRE(queries && gallery, "rank: null queries/gallery pointer");
    MI355_REQUIRE(Q >= 1, "rank: Q=%lld must be >= 1", (long long)Q);
    MI355_REQUIRE(G >= 1, "rank: G=%lld must be >= 1", (long long)G);
    MI355_REQUIRE(dim >= 1, "rank: dim=%d must be >= 1", dim);
    return OK;
}
// mi355_rank_topk and mi355_rank_topk_filtered, under the name who
static int check_topk_args(const float* queries, i64 Q, const float* gallery, i64 G, int dim, int k, const float* out_val,
                           const int64_t* out_idx, const char* who) {
    if (int e = check_rank_args(queries, Q, gallery, G, dim)) return e;
    MI355_REQUIRE(out_val && out_idx, "%s: null output", who);
    MI355_REQUIRE(k >= 1 && k <= LARGE_K, "%s: k=%d outside [1,%d]", who, k, LARGE_K);
    MI355_REQUIRE(k <= G, "%s: k=%d exceeds gallery rows %lld", who, k, (long long)G);
    return OK;
}

// mi355_rank_topk and, with filt, mi355_rank_topk_filtered (arguments checked by the caller)
static int rank_topk(const float* queries, i64 Q, const float* gallery, i64 G, int dim, int gallery_is_normalized, int k, float eps,
                     i64 idx_offset, float* out_val, i64* out_idx, void* workspace, size_t workspace_bytes, hipStream_t st,
                     const RankFilter* filt) {
    const RankWs w = carve(workspace, Q, G, dim, k, split_queries_bytes, !gallery_is_normalized);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "rank_topk: workspace %zu < %zu bytes", workspace_bytes,
                  w.total);
    const float* ginv = gallery_is_normalized ? nullptr : w.ginv;
    return search_blocks(queries, ginv ? gallery : nullptr, Q, G, dim, k, eps, idx_offset, filt, out_val, out_idx, w, st, nullptr,
                         [&](i64 q0, i64 qn, const RankFilter* f) -> int {
                             RoctxRange range(w.cand_val ? "rank/cosine gemm + per-tile top-k" : nullptr);
                             return with_topk_epi(w, k, f, [&](const auto& epi) {
                                 return cos_gemm(w.qn + q0 * dim, (bf16_t*)w.qs, gallery, ginv, qn, G, dim, epi, st);
                             });
                         });
}

// ---- the searches without a top-k, once for fp32 and fp16 rows (rank_common.h)
GalleryRows f32_rows(const float* gallery, int is_normalized) {
    return {gallery, is_normalized != 0, nullptr, 0, split_queries_bytes};
}
static int check_rows(const GalleryRows& g, const char* who) {
    MI355_REQUIRE((((uintptr_t)g.f16 | (uintptr_t)g.i8 | (uintptr_t)g.fp4) & 15) == 0, "%s: gallery buffer must be 16-byte aligned", who);
    return OK;
}
// The normalised queries qn [Q][dim] (qs: scratch of g.planes_bytes(Q, dim)) against the rows of g with epilogue epi
template <class Epi>
static int score_rows(const GalleryRows& g, const float* ginv, const float* qn, void* qs, i64 Q, i64 G, int dim, const Epi& epi,
                      hipStream_t st) {
    if (g.f16) return cos_gemm_f16(g.f16, g.ld, qn, qs, Q, G, dim, epi, st);
    if constexpr (std::is_same_v<Epi, RangeArgs>) {      // int8 and fp4 rows: the range search only
        if (g.i8) return cos_gemm_i8(g.i8, g.scales, g.ld, qn, qs, Q, G, dim, epi, st);
        if (g.fp4) return cos_gemm_fp4(g.fp4, g.scales, g.ld, qn, qs, Q, G, dim, epi, st);
    }
    return cos_gemm(qn, (bf16_t*)qs, g.f32, ginv, Q, G, dim, epi, st);
}

// fn(the epilogue of one GEMM call of an adjusted search over the scratch w): with_topk_epi with the map in front of the
// selection, or the adjusted slab
template <class Fn>
static int with_adjusted_epi(const RankWs& w, int k, const RankFilter* f, const ScoreAdjust& adj, Fn&& fn) {
    if (!w.cand_val) return fn(AdjSlabEpi{w.S, adj});
    if (f) return with_adjusted_select_epi<true>(k, w.cand_val, w.cand_idx, *f, adj, fn);
    return with_adjusted_select_epi<false>(k, w.cand_val, w.cand_idx, RankFilter{}, adj, fn);
}

// The block loop is search_blocks' with the adjustment shifted beside the filter; the caller's query_block only shortens it
int adjusted_search(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, int k, i64 idx_offset,
                    const ScoreAdjust& adj, const RankFilter* filt, i64 query_block_arg, float* out_val, i64* out_idx, void* workspace,
                    size_t workspace_bytes, hipStream_t st, const char* who) {
    const bool need_ginv = g.f32 && !g.unit;
    const RankWs w = carve(workspace, Q, G, dim, k, g.planes_bytes, need_ginv, k > 0);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    const float* ginv = need_ginv ? w.ginv : nullptr;
    if (int e = normalize_search(queries, Q, ginv ? g.f32 : nullptr, G, dim, eps, w, st)) return e;
    const bool fused = fused_select(Q, G, k);
    i64 qb = k > 0 ? query_block(Q, G, k) : (Q < 256 * 64 ? Q : 256 * 64);
    if (query_block_arg > 0 && query_block_arg < qb) qb = query_block_arg;
    const i64 rowlen = fused ? cdiv(G, RK_BN) * (i64)k : G;
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = (Q - q0 < qb) ? Q - q0 : qb;
        const ScoreAdjust ab = adjust_from(adj, q0);
        if (k == 0) {
            RoctxRange range("scorenorm/cosine gemm + adjusted slab");
            if (int e = score_rows(g, ginv, w.qn + q0 * dim, w.qs, qn, G, dim, AdjSlabEpi{out_val + q0 * G, ab}, st)) return e;
            continue;
        }
        const RankFilter fb = filt ? filter_from(*filt, q0) : RankFilter{};
        const RankFilter* f = filt ? &fb : nullptr;
        {
            RoctxRange range(fused ? "scorenorm/cosine gemm + adjusted per-tile top-k" : "scorenorm/cosine gemm + adjusted slab");
            if (int e = with_adjusted_epi(w, k, f, ab, [&](const auto& epi) {
                    return score_rows(g, ginv, w.qn + q0 * dim, w.qs, qn, G, dim, epi, st);
                }))
                return e;
        }
        if (!fused && k > SMALL_K) set_rank_path(mi355_rank_last_path() | MI355_RANK_PATH_BITONIC);
        RoctxRange range(fused ? "rank/merge candidates" : "rank/top-k");
        if (int e = topk_select(fused ? w.cand_val : w.S, nullptr, qn, rowlen, rowlen, k, idx_offset, out_val + q0 * k, out_idx + q0 * k,
                                w.topk, w.topk_bytes, st, w.cand_idx, f))
            return e;
    }
    return OK;
}

int roc_pairs_hist(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, const int64_t* query_labels,
                   const int64_t* gallery_labels, const int64_t* exclude, i64 idx_offset, const double* thresholds,
                   const double* thresholds_dev, int T, int64_t* hist, void* workspace, size_t workspace_bytes, size_t need,
                   void* stream, const char* who) {
    RocArgs roc{};
    if (int e = roc_check_thresholds(thresholds, T, who, &roc)) return e;
    if (int e = roc_check_pairs(query_labels, gallery_labels, exclude, idx_offset, thresholds_dev, hist, who, &roc)) return e;
    MI355_REQUIRE(queries && g.rows(), "%s: null queries/gallery pointer", who);
    MI355_REQUIRE(Q >= 1 && G >= 1 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    if (int e = check_rows(g, who)) return e;
    MI355_REQUIRE(Q <= INT_MAX && G < ((int64_t)1 << 31) - RK_BN, "%s: shape too large Q=%lld G=%lld", who, (long long)Q,
                  (long long)G);
    MI355_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    const RankWs w = carve(workspace, Q, G, dim, 0, g.planes_bytes, g.f32 && !g.unit, false);
    hipStream_t st = (hipStream_t)stream;
    MI355_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)2 * (T + 1) * sizeof(int64_t), st));
    const float* ginv = g.f32 && !g.unit ? w.ginv : nullptr;
    if (int e = normalize_search(queries, Q, ginv ? g.f32 : nullptr, G, dim, eps, w, st)) return e;
    const i64 qb = roc_query_block(Q, G);
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = (Q - q0 < qb) ? Q - q0 : qb;
        RoctxRange range(g.f16 ? "roc/cosine gemm (fp16 gallery) + histogram" : "roc/cosine gemm + histogram");
        if (int e = score_rows(g, ginv, w.qn + q0 * dim, w.qs, qn, G, dim, roc_from(roc, q0), st)) return e;
    }
    return OK;
}

// candidates: [2][capacity] entries, raw hits of one GEMM call (in reservation order) then the canonical CSR payload of the
// whole call.  Per query block: zero the cursor, run the range pass, read the block's hit count back (the one host sync), and
// while everything so far fits compact the block.  Once a block does not fit, the rest only count (cap 0): *nnz is the exact
// total either way, and a call with capacity >= *nnz fits.
int cosine_range(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, double threshold, i64 idx_offset,
                 const mi355_rank_filter* filter, void* candidates, i64 capacity, int64_t* nnz, void* workspace,
                 size_t workspace_bytes, void* stream, bool keep_all, const char* who) {
    RankFilter f{};
    if (int e = range_check(queries, Q, g.rows(), G, dim, threshold, filter, idx_offset, candidates, capacity, nnz, who, &f)) return e;
    if (int e = check_rows(g, who)) return e;
    const RangeWs w = range_carve(workspace, Q, G, dim, g.planes_bytes, g.f32 && !g.unit);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    if (Q == 0 || G == 0) return range_empty(w, Q, nnz, st);
    const float* ginv = g.f32 && !g.unit ? w.w.ginv : nullptr;
    if (int e = normalize_search(queries, Q, ginv ? g.f32 : nullptr, G, dim, eps, w.w, st)) return e;
    unsigned long long* raw = (unsigned long long*)candidates;
    unsigned long long* canon = raw ? raw + capacity : nullptr;
    MI355_CHECK_HIP(hipMemsetAsync(w.offsets, 0, sizeof(i64), st));
    const i64 qb = range_query_block(Q, G);
    i64 off = 0;
    bool fits = true;
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = (Q - q0 < qb) ? Q - q0 : qb;
        MI355_CHECK_HIP(hipMemsetAsync(w.cursor, 0, sizeof(unsigned long long), st));
        const RangeArgs a{filter_from(f, q0), roc_ceil_f32(threshold), w.cursor, raw, fits ? capacity : 0, w.tstart, w.tcount,
                          keep_all ? 1 : 0};
        {
            RoctxRange range(keep_all ? "ranks/positives" : g.f16 ? "range/cosine gemm (fp16 gallery) + hits"
                             : g.i8 ? "range/cosine gemm (int8 gallery) + hits"
                             : g.fp4 ? "range/cosine gemm (fp4 gallery) + hits" : "range/cosine gemm + hits");
            if (int e = score_rows(g, ginv, w.w.qn + q0 * dim, w.w.qs, qn, G, dim, a, st)) return e;
        }
        unsigned long long n = 0;
        MI355_CHECK_HIP(hipMemcpyAsync(&n, w.cursor, sizeof(n), hipMemcpyDeviceToHost, st));
        MI355_CHECK_HIP(hipStreamSynchronize(st));
        fits = fits && off + (i64)n <= capacity;
        if (fits) {
            RoctxRange range("range/compact");
            if (int e = range_compact_block(w, q0, qn, G, off, raw, canon, st)) return e;
        }
        off += (i64)n;
    }
    *nnz = off;
    return OK;
}

int rank_positives(const float* queries, i64 Q, const GalleryRows& g, i64 G, int dim, float eps, const int64_t* query_labels,
                   const int64_t* gallery_labels, const int64_t* exclude, i64 idx_offset, const int64_t* offsets,
                   const int64_t* offsets_host, const uint64_t* pos_keys, i64 nnz, uint32_t* before, i64 query_block,
                   void* workspace, size_t workspace_bytes, size_t need, void* stream, const char* who) {
    RanksArgs rk{};
    if (int e = ranks_check(queries, Q, g.rows(), G, dim, query_labels, gallery_labels, exclude, idx_offset, offsets, offsets_host,
                            pos_keys, nnz, before, query_block, who, &rk))
        return e;
    if (int e = check_rows(g, who)) return e;
    MI355_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    const RankWs w = carve(workspace, Q, G, dim, 0, g.planes_bytes, g.f32 && !g.unit, false);
    hipStream_t st = (hipStream_t)stream;
    if (nnz == 0) return OK;                                    // no query has a positive: nothing to count
    MI355_CHECK_HIP(hipMemsetAsync(before, 0, (size_t)nnz * sizeof(uint32_t), st));
    const float* ginv = g.f32 && !g.unit ? w.ginv : nullptr;
    if (int e = normalize_search(queries, Q, ginv ? g.f32 : nullptr, G, dim, eps, w, st)) return e;
    const i64 qb = ranks_query_block(Q, G, query_block);
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = (Q - q0 < qb) ? Q - q0 : qb;
        RoctxRange range("ranks/count");
        if (int e = score_rows(g, ginv, w.qn + q0 * dim, w.qs, qn, G, dim, ranks_from(rk, q0), st)) return e;
    }
    return OK;
}

// best[] -> assign (the centroid in the low word, complemented) and score (the fp32 the key was made from; -0 reads as +0)
__global__ __launch_bounds__(256) void k_nearest_unpack(const unsigned long long* __restrict__ best, i64 G, i64* __restrict__ assign,
                                                        float* __restrict__ score) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < G; i += stride) {
        const unsigned long long e = best[i];
        assign[i] = (i64)(unsigned)~(unsigned)(e & 0xffffffffull);
        score[i] = key_score((unsigned)(e >> 32));
    }
}

size_t nearest_ws_bytes(i64 K, i64 G, int dim, size_t (*planes_bytes)(i64, int), bool need_ginv) {
    return align_up((size_t)G * sizeof(unsigned long long), 256) + carve(nullptr, K, G, dim, 0, planes_bytes, need_ginv, false).total;
}

int nearest_centroid(const float* centroids, i64 K, const GalleryRows& g, i64 G, int dim, float eps, i64 query_block,
                     int64_t* assign, float* score, void* workspace, size_t workspace_bytes, void* stream, const char* who) {
    MI355_REQUIRE(centroids && g.rows(), "%s: null centroids/rows pointer", who);
    MI355_REQUIRE(assign && score, "%s: null assign/score output", who);
    MI355_REQUIRE(K >= 1 && G >= 1 && dim >= 1, "%s: bad shape K=%lld N=%lld dim=%d", who, (long long)K, (long long)G, dim);
    if (int e = check_rows(g, who)) return e;
    MI355_REQUIRE(K <= INT_MAX && G < ((int64_t)1 << 31) - RK_BN, "%s: shape too large K=%lld N=%lld", who, (long long)K,
                  (long long)G);
    MI355_REQUIRE(query_block >= 0, "%s: query_block=%lld < 0", who, (long long)query_block);
    const size_t need = nearest_ws_bytes(K, G, dim, g.planes_bytes, g.f32 && !g.unit);
    MI355_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    char* base = align256(workspace);
    unsigned long long* best = (unsigned long long*)base;
    const RankWs w = carve(base + align_up((size_t)G * sizeof(unsigned long long), 256), K, G, dim, 0, g.planes_bytes,
                           g.f32 && !g.unit, false);
    hipStream_t st = (hipStream_t)stream;
    MI355_CHECK_HIP(hipMemsetAsync(best, 0, (size_t)G * sizeof(unsigned long long), st));
    const float* ginv = g.f32 && !g.unit ? w.ginv : nullptr;
    if (int e = normalize_search(centroids, K, ginv ? g.f32 : nullptr, G, dim, eps, w, st)) return e;
    const i64 qb = ranks_query_block(K, G, query_block);
    for (i64 q0 = 0; q0 < K; q0 += qb) {
        const i64 qn = (K - q0 < qb) ? K - q0 : qb;
        RoctxRange range(g.f16 ? "kmeans/cosine gemm (fp16 rows) + nearest centroid" : "kmeans/cosine gemm + nearest centroid");
        if (int e = score_rows(g, ginv, w.qn + q0 * dim, w.qs, qn, G, dim, NearestEpi{best, (int)q0}, st)) return e;
    }
    const unsigned blocks = (unsigned)(cdiv(G, 256) < 8192 ? cdiv(G, 256) : 8192);
    hipLaunchKernelGGL(k_nearest_unpack, dim3(blocks), dim3(256), 0, st, (const unsigned long long*)best, G, (i64*)assign, score);
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t dbscan_ws_bytes(i64 rows, i64 N, int dim, size_t (*planes_bytes)(i64, int), bool need_ginv) {
    return carve(nullptr, rows, N, dim, 0, planes_bytes, need_ginv, false).total;
}

int dbscan_sweep(const float* queries, i64 q0, i64 rows, const GalleryRows& g, i64 N, int dim, float eps, double threshold,
                 int min_samples, int32_t* degree, int32_t* parent, uint64_t* border, bool link, void* workspace,
                 size_t workspace_bytes, void* stream, const char* who) {
    if (int e = dbscan_check(queries, q0, rows, g.rows(), N, dim, threshold, min_samples, degree, parent, border, link, who)) return e;
    if (int e = check_rows(g, who)) return e;
    const size_t need = dbscan_ws_bytes(rows, N, dim, g.planes_bytes, g.f32 && !g.unit);
    MI355_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    if (rows == 0) return OK;
    const RankWs w = carve(workspace, rows, N, dim, 0, g.planes_bytes, g.f32 && !g.unit, false);
    hipStream_t st = (hipStream_t)stream;
    const float* ginv = g.f32 && !g.unit ? w.ginv : nullptr;
    if (int e = normalize_search(queries, rows, ginv ? g.f32 : nullptr, N, dim, eps, w, st)) return e;
    const float thr = roc_ceil_f32(threshold);
    const i64 qb = roc_query_block(rows, N);
    for (i64 b0 = 0; b0 < rows; b0 += qb) {
        const i64 qn = (rows - b0 < qb) ? rows - b0 : qb;
        RoctxRange range(link ? "dbscan/cosine gemm + link" : "dbscan/cosine gemm + degree");
        if (link) {
            const LinkEpi epi{thr, (int)(q0 + b0), min_samples, degree, parent, (unsigned long long*)border};
            if (int e = score_rows(g, ginv, w.qn + b0 * dim, w.qs, qn, N, dim, epi, st)) return e;
        } else {
            if (int e = score_rows(g, ginv, w.qn + b0 * dim, w.qs, qn, N, dim, DegreeEpi{thr, degree + q0 + b0}, st)) return e;
        }
    }
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_l2_normalize_rows(const float* in, float* out, int64_t rows, int dim, float eps, void* stream) {
    MI355_REQUIRE(in && out, "l2_normalize_rows: null pointer");
    MI355_REQUIRE(rows >= 0 && dim >= 1, "l2_normalize_rows: bad shape rows=%lld dim=%d", (long long)rows, dim);
    if (rows == 0) return OK;
    const int vec = vec_ok(in, dim) && vec_ok(out, dim);
    hipLaunchKernelGGL((k_row_norm<true>), dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, in, out,
                       (float*)nullptr, (i64)rows, dim, eps, vec);
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t mi355_rank_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || G < 1) return 0;
    if (dim <= 0) return topk_ws_bytes(Q, G, k < 1 ? 1 : k) + 256;
    return carve(nullptr, Q, G, dim, k, split_queries_bytes, true).total;
}

int mi355_cosine_scores(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim,
                        int gallery_is_normalized, float eps, float* out, void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (int e = check_rank_args(queries, Q, gallery, G, dim)) return e;
    MI355_REQUIRE(out, "cosine_scores: null output");
    hipStream_t st = (hipStream_t)stream;
    RankWs w = carve(workspace, Q, G, dim, 0, split_queries_bytes, !gallery_is_normalized, false);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "cosine_scores: workspace %zu < %zu bytes",
                  workspace_bytes, w.total);
    const float* ginv = gallery_is_normalized ? nullptr : w.ginv;
    if (int e = normalize_search(queries, Q, ginv ? gallery : nullptr, G, dim, eps, w, st)) return e;
    for (i64 qs = 0; qs < Q; qs += 256 * 64) {  // grid.y stays small
        const i64 qn = (Q - qs < 256 * 64) ? Q - qs : 256 * 64;
        if (int e = cos_gemm(w.qn + qs * dim, (bf16_t*)w.qs, gallery, ginv, qn, G, dim, SlabEpi{out + qs * G}, st)) return e;
    }
    return OK;
}

int mi355_rank_topk(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim,
                    int gallery_is_normalized, int k, float eps, int64_t idx_offset, float* out_val,
                    int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = check_topk_args(queries, Q, gallery, G, dim, k, out_val, out_idx, "rank_topk")) return e;
    return rank_topk(queries, Q, gallery, G, dim, gallery_is_normalized, k, eps, idx_offset, out_val, (i64*)out_idx, workspace,
                     workspace_bytes, (hipStream_t)stream, nullptr);
}

int mi355_rank_topk_filtered(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim,
                             int gallery_is_normalized, int k, float eps, int64_t idx_offset, const mi355_rank_filter* filter,
                             float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = check_topk_args(queries, Q, gallery, G, dim, k, out_val, out_idx, "rank_topk_filtered")) return e;
    RankFilter f{};
    if (int e = make_filter(filter, idx_offset, "rank_topk_filtered", &f)) return e;
    return rank_topk(queries, Q, gallery, G, dim, gallery_is_normalized, k, eps, idx_offset, out_val, (i64*)out_idx, workspace,
                     workspace_bytes, (hipStream_t)stream, &f);
}

int mi355_rank_last_path(void) { return g_rank_path; }

int mi355_rank_round_split(int ntx, int ny, int slots) {
    if (ntx < 0 || ny < 1 || slots < 1) return -1;
    return whole_round_tiles(ntx, ny, slots);
}

int mi355_rank_set_round_slots(int slots) {
    MI355_REQUIRE(slots >= 0, "rank_set_round_slots: slots=%d must be >= 0 (0: the device's own count)", slots);
    g_round_slots = slots;
    return OK;
}

int mi355_rank_last_tiles(int* out, int n) {
    if (!out || n < 1) return -1;
    const int m = n < 5 ? n : 5;
    for (int i = 0; i < m; ++i) out[i] = g_last_tiles[i];
    return m;
}

size_t mi355_roc_pairs_workspace_bytes(int64_t Q, int64_t G, int dim) {
    if (Q < 1 || G < 1 || dim < 1) return 0;
    // the normalised queries, the split planes of one GEMM call (roc_query_block <= 256 * 64 queries), 1 / |row| of the
    // gallery rows: no slab, no candidates
    return carve(nullptr, Q, G, dim, 0, split_queries_bytes, true, false).total;
}

int mi355_roc_pairs_hist(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                         float eps, const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude,
                         int64_t idx_offset, const double* thresholds, const double* thresholds_dev, int T, int64_t* hist,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return roc_pairs_hist(queries, Q, f32_rows(gallery, gallery_is_normalized), G, dim, eps, query_labels, gallery_labels, exclude,
                          idx_offset, thresholds, thresholds_dev, T, hist, workspace, workspace_bytes,
                          mi355_roc_pairs_workspace_bytes(Q, G, dim), stream, "roc_pairs_hist");
}

size_t mi355_range_workspace_bytes(int64_t Q, int64_t G, int dim) {
    if (Q < 0 || G < 0 || dim < 1) return 0;
    return range_carve(nullptr, Q, G, dim, split_queries_bytes, true).total;
}

int mi355_cosine_range(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                       float eps, double threshold, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates,
                       int64_t capacity, int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_range(queries, Q, f32_rows(gallery, gallery_is_normalized), G, dim, eps, threshold, idx_offset, filter, candidates,
                        capacity, nnz, workspace, workspace_bytes, stream, false, "cosine_range");
}

int mi355_positives_range(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                          float eps, int64_t idx_offset, const mi355_rank_filter* filter, void* candidates, int64_t capacity,
                          int64_t* nnz, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(filter && filter->label_mode == MI355_LABEL_SAME, "positives_range: needs a filter with MI355_LABEL_SAME");
    return cosine_range(queries, Q, f32_rows(gallery, gallery_is_normalized), G, dim, eps, 0.0, idx_offset, filter, candidates,
                        capacity, nnz, workspace, workspace_bytes, stream, true, "positives_range");
}

size_t mi355_rank_positives_workspace_bytes(int64_t Q, int64_t G, int dim) { return mi355_roc_pairs_workspace_bytes(Q, G, dim); }

int mi355_rank_positives(const float* queries, int64_t Q, const float* gallery, int64_t G, int dim, int gallery_is_normalized,
                         float eps, const int64_t* query_labels, const int64_t* gallery_labels, const int64_t* exclude,
                         int64_t idx_offset, const int64_t* offsets, const int64_t* offsets_host, const uint64_t* pos_keys,
                         int64_t nnz, uint32_t* before, int64_t query_block, void* workspace, size_t workspace_bytes,
                         void* stream) {
    return rank_positives(queries, Q, f32_rows(gallery, gallery_is_normalized), G, dim, eps, query_labels, gallery_labels, exclude,
                          idx_offset, offsets, offsets_host, pos_keys, nnz, before, query_block, workspace, workspace_bytes,
                          mi355_rank_positives_workspace_bytes(Q, G, dim), stream, "rank_positives");
}

size_t mi355_nearest_centroid_workspace_bytes(int64_t K, int64_t N, int dim) {
    if (K < 1 || N < 1 || dim < 1) return 0;
    return nearest_ws_bytes(K, N, dim, split_queries_bytes, true);
}

int mi355_nearest_centroid(const float* centroids, int64_t K, const float* rows, int64_t N, int dim, int rows_are_normalized, float eps,
                           int64_t query_block, int64_t* assign, float* score, void* workspace, size_t workspace_bytes,
                           void* stream) {
    return nearest_centroid(centroids, K, f32_rows(rows, rows_are_normalized), N, dim, eps, query_block, assign, score, workspace,
                            workspace_bytes, stream, "nearest_centroid");
}

size_t mi355_dbscan_workspace_bytes(int64_t rows, int64_t N, int dim) {
    if (rows < 1 || N < 1 || dim < 1) return 0;
    return dbscan_ws_bytes(rows, N, dim, split_queries_bytes, true);
}

int mi355_dbscan_degree(const float* queries, int64_t q0, int64_t rows, const float* gallery, int64_t N, int dim,
                        int gallery_is_normalized, float eps, double threshold, int32_t* degree, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return dbscan_sweep(queries, q0, rows, f32_rows(gallery, gallery_is_normalized), N, dim, eps, threshold, 1, degree, nullptr,
                        nullptr, false, workspace, workspace_bytes, stream, "dbscan_degree");
}

int mi355_dbscan_link(const float* queries, int64_t q0, int64_t rows, const float* gallery, int64_t N, int dim,
                      int gallery_is_normalized, float eps, double threshold, int min_samples, const int32_t* degree,
                      int32_t* parent, uint64_t* border, void* workspace, size_t workspace_bytes, void* stream) {
    return dbscan_sweep(queries, q0, rows, f32_rows(gallery, gallery_is_normalized), N, dim, eps, threshold, min_samples,
                        const_cast<int32_t*>(degree), parent, border, true, workspace, workspace_bytes, stream, "dbscan_link");
}

int mi355_clear_pads(float* val, int64_t* idx, int64_t n, int64_t lo, int64_t hi, void* stream) {
    MI355_REQUIRE(val && idx, "clear_pads: null pointer");
    MI355_REQUIRE(n >= 0, "clear_pads: n=%lld < 0", (long long)n);
    if (n == 0) return OK;
    hipLaunchKernelGGL(k_clear_pads, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, val, (i64*)idx, (i64)n,
                       (i64)lo, (i64)hi);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_retrieval_metrics(const int64_t* idx, int64_t Q, int k, const int64_t* query_cls, const int64_t* gallery_cls,
                            int64_t G, const int64_t* R, double* per_query, void* stream) {
    MI355_REQUIRE(idx && query_cls && gallery_cls && R && per_query, "retrieval_metrics: null pointer");
    MI355_REQUIRE(Q >= 1 && G >= 1, "retrieval_metrics: bad shape Q=%lld G=%lld", (long long)Q, (long long)G);
    MI355_REQUIRE(k >= 1 && k <= LARGE_K, "retrieval_metrics: k=%d outside [1,%d]", k, LARGE_K);
    hipLaunchKernelGGL(k_retrieval_metrics, dim3((unsigned)cdiv(Q, 4)), dim3(256), 0, (hipStream_t)stream, (const i64*)idx, (i64)Q,
                       k, (const i64*)query_cls, (const i64*)gallery_cls, (i64)G, (const i64*)R, per_query);
    MI355_LAUNCH_CHECK();
    return OK;
}

// ---- prepared gallery (resident galleries: Gallery / ShardedGallery hold it next to nothing else for k <= 8 searches)
// planes of the NORMALISED rows, in the fragment order of the GEMM's B operand: whole 128-row tiles, 16-deep k steps, 6 B per element
size_t mi355_gallery_planes_bytes(int64_t G, int dim) {
    if (G < 1 || dim < 1) return 0;
    return split_queries_bytes(G, dim);
}

int mi355_gallery_prepare(const float* gallery_normalized, int64_t G, int dim, void* planes, size_t planes_bytes, void* stream) {
    MI355_REQUIRE(gallery_normalized && planes, "gallery_prepare: null pointer");
    MI355_REQUIRE(G >= 1 && dim >= 1 && G < ((int64_t)1 << 31) - RK_BN, "gallery_prepare: bad shape G=%lld dim=%d", (long long)G, dim);
    MI355_REQUIRE(planes_bytes >= mi355_gallery_planes_bytes(G, dim), "gallery_prepare: planes buffer %zu < %zu bytes", planes_bytes,
                  mi355_gallery_planes_bytes(G, dim));
    MI355_REQUIRE((i64)cdiv(G, 128) * 4 * cdiv(dim, 16) < ((i64)1 << 31), "gallery_prepare: gallery too large for one call");
    return split_rows(gallery_normalized, G, dim, (bf16_t*)planes, (hipStream_t)stream);
}

// mi355_rank_topk against a prepared gallery (rows normalised when the planes were made): k <= 8, Q > 4 (the fused selection's
// range; other shapes go through mi355_rank_topk with the fp32 rows).  Scores and indices are bit-identical to
// mi355_rank_topk(gallery_is_normalized = 1) on the same rows.  workspace: mi355_rank_workspace_bytes(Q, G, dim, k).
int mi355_rank_topk_prepared(const float* queries, int64_t Q, const void* gallery_planes, int64_t G, int dim, int k, float eps,
                             int64_t idx_offset, float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                             void* stream) {
    MI355_REQUIRE(queries && gallery_planes && out_val && out_idx, "rank_topk_prepared: null pointer");
    MI355_REQUIRE(Q >= 1 && G >= 1 && dim >= 1, "rank_topk_prepared: bad shape Q=%lld G=%lld dim=%d", (long long)Q, (long long)G, dim);
    MI355_REQUIRE(k >= 1 && k <= G, "rank_topk_prepared: k=%d outside [1, %lld]", k, (long long)G);
    MI355_REQUIRE(fused_select(Q, G, k), "rank_topk_prepared: needs k <= %d and more than 4 queries (got k=%d, Q=%lld)", SMALL_K, k, (long long)Q);
    hipStream_t st = (hipStream_t)stream;
    const RankWs w = carve(workspace, Q, G, dim, k, split_queries_bytes, false);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "rank_topk_prepared: workspace %zu < %zu bytes", workspace_bytes, w.total);
    return search_blocks(queries, nullptr, Q, G, dim, k, eps, idx_offset, nullptr, out_val, (i64*)out_idx, w, st, nullptr,
                         [&](i64 q0, i64 qn, const RankFilter*) -> int {
                             RoctxRange range("rank/cosine gemm (prepared gallery) + per-tile top-k");
                             if (int e = split_rows(w.qn + q0 * dim, qn, dim, (bf16_t*)w.qs, st)) return e;
                             set_rank_path(MI355_RANK_PATH_PREPARED | MI355_RANK_PATH_FUSED);
                             return with_select_epi<false>(k, w.cand_val, w.cand_idx, RankFilter{}, [&](const auto& epi) {
                                 return cos_gemm_tiles<PreparedGemm>({w.qs, gallery_planes, nullptr, (int)qn, G, dim}, epi, st);
                             });
                         });
}

int mi355_topk_rows(const float* scores, int64_t Q, int64_t G, int k, int64_t idx_offset, float* out_val,
                    int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(scores && out_val && out_idx, "topk_rows: null pointer");
    MI355_REQUIRE(Q >= 1 && G >= 1, "topk_rows: bad shape Q=%lld G=%lld", (long long)Q, (long long)G);
    MI355_REQUIRE(workspace, "topk_rows: null workspace");
    return topk_select(scores, nullptr, Q, G, G, k, idx_offset, out_val, (i64*)out_idx, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int mi355_merge_topk(const float* cand_val, const int64_t* cand_idx, int64_t Q, int ncand, int k, float* out_val,
                     int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(cand_val && cand_idx && out_val && out_idx, "merge_topk: null pointer");
    MI355_REQUIRE(Q >= 1 && ncand >= 1, "merge_topk: bad shape Q=%lld ncand=%d", (long long)Q, ncand);
    MI355_REQUIRE(workspace, "merge_topk: null workspace");
    return topk_select(cand_val, (const i64*)cand_idx, Q, ncand, ncand, k, 0, out_val, (i64*)out_idx, workspace,
                       workspace_bytes, (hipStream_t)stream);
}

// ---- packed candidates of the sharded search (sharded.py): ONE int32 tensor per rank travels through the all-gather.
// packed[q][j] = {bits of the f32 score, LOCAL row index}; slots j >= kk (a shard with fewer than k rows) = {-inf, -1}.
int mi355_pack_candidates(const float* val, const int64_t* idx, int64_t Q, int kk, int k, int32_t* packed, void* stream) {
    MI355_REQUIRE(packed && Q >= 1 && k >= 1 && kk >= 0 && kk <= k, "pack_candidates: bad arguments Q=%lld kk=%d k=%d",
                  (long long)Q, kk, k);
    MI355_REQUIRE(kk == 0 || (val && idx), "pack_candidates: null candidates");
    const i64 n = (i64)Q * k;
    hipLaunchKernelGGL(k_pack_candidates, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, val,
                       (const i64*)idx, (i64)Q, kk, k, packed);
    MI355_LAUNCH_CHECK();
    return OK;
}

// Merge of the all-gathered packed candidates [world][Q][k][2]: the shard offsets (device, int64[world]) are added here and
// the world * k candidates of a query are merged with the rule of every other selection (higher score, then LOWER global
// index) -> (Q, k) identical to the unsharded result.  workspace: mi355_merge_packed_workspace_bytes(Q, world, k).
size_t mi355_merge_packed_workspace_bytes(int64_t Q, int world, int k) {
    if (Q < 1 || world < 1 || k < 1) return 0;
    const size_t n = (size_t)Q * world * k;
    return align_up(n * sizeof(i64), 256) + align_up(n * sizeof(float), 256) + topk_ws_bytes(Q, (i64)world * k, k) + 512;
}

int mi355_merge_packed_topk(const int32_t* packed, const int64_t* shard_offsets, int world, int64_t Q, int k,
                            float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(packed && shard_offsets && out_val && out_idx, "merge_packed_topk: null pointer");
    MI355_REQUIRE(Q >= 1 && world >= 1 && k >= 1, "merge_packed_topk: bad shape Q=%lld world=%d k=%d", (long long)Q, world, k);
    MI355_REQUIRE(workspace && workspace_bytes >= mi355_merge_packed_workspace_bytes(Q, world, k),
                  "merge_packed_topk: workspace %zu < %zu bytes", workspace_bytes, mi355_merge_packed_workspace_bytes(Q, world, k));
    const size_t n = (size_t)Q * world * k;
    char* base = align256(workspace);
    i64* ci = (i64*)base;
    float* cv = (float*)(base + align_up(n * sizeof(i64), 256));
    char* rest = base + align_up(n * sizeof(i64), 256) + align_up(n * sizeof(float), 256);
    hipLaunchKernelGGL(k_unpack_candidates, dim3((unsigned)cdiv((i64)n, 256)), dim3(256), 0, (hipStream_t)stream, packed,
                       (const i64*)shard_offsets, world, (i64)Q, k, cv, ci);
    MI355_LAUNCH_CHECK();
    return topk_select(cv, ci, Q, (i64)world * k, (i64)world * k, k, 0, out_val, (i64*)out_idx, rest,
                       workspace_bytes - (size_t)(rest - (char*)workspace), (hipStream_t)stream);
}

int mi355_pair_cosine(const float* a, const float* b, int64_t rows, int dim, float eps, float* out, void* stream) {
    MI355_REQUIRE(a && b && out, "pair_cosine: null pointer");
    MI355_REQUIRE(rows >= 0 && dim >= 1, "pair_cosine: bad shape");
    if (rows == 0) return OK;
    hipLaunchKernelGGL(k_pair_cosine, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, a, b,
                       (i64)rows, dim, eps, out);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_contrastive_loss(const float* fm1, const float* fm2, int64_t rows, int dim, float label, float margin,
                           int mean, float* out, float* per_row, void* stream) {
    MI355_REQUIRE(fm1 && fm2 && out, "contrastive_loss: null pointer");
    MI355_REQUIRE(rows >= 1 && dim >= 1, "contrastive_loss: bad shape rows=%lld dim=%d", (long long)rows, dim);
    hipLaunchKernelGGL(k_contrastive, dim3(1), dim3(1024), 0, (hipStream_t)stream, fm1, fm2, (i64)rows, dim, label,
                       margin, mean, out, per_row);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_cosine_embedding_loss(const float* x1, const float* x2, int64_t rows, int dim, float target, float margin,
                                int mean, float* out, void* stream) {
    MI355_REQUIRE(x1 && x2 && out, "cosine_embedding_loss: null pointer");
    MI355_REQUIRE(rows >= 1 && dim >= 1, "cosine_embedding_loss: bad shape rows=%lld dim=%d", (long long)rows, dim);
    MI355_REQUIRE(target == 1.0f || target == -1.0f, "cosine_embedding_loss: target must be +1 or -1");
    hipLaunchKernelGGL(k_cos_embedding_loss, dim3(1), dim3(1024), 0, (hipStream_t)stream, x1, x2, (i64)rows, dim, target,
                       margin, mean, out);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_hit_counts(const int64_t* idx, int64_t Q, int k, const int64_t* query_cls, const int64_t* gallery_cls,
                     int64_t G, int64_t* counts, void* stream) {
    MI355_REQUIRE(idx && query_cls && gallery_cls && counts, "hit_counts: null pointer");
    MI355_REQUIRE(Q >= 1 && k >= 1 && G >= 1, "hit_counts: bad shape");
    hipLaunchKernelGGL(k_hit_counts, dim3((unsigned)cdiv(Q, 256)), dim3(256), 0, (hipStream_t)stream, (const i64*)idx,
                       (i64)Q, k, (const i64*)query_cls, (const i64*)gallery_cls, (i64)G, (i64*)counts);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_distinct_class_topn(const int64_t* idx, const float* val, int64_t Q, int k, const int64_t* gallery_cls,
                              int64_t G, int n, int64_t* out_cls, int64_t* out_idx, float* out_val, void* stream) {
    MI355_REQUIRE(idx && val && gallery_cls && out_cls && out_idx && out_val, "distinct_class_topn: null pointer");
    MI355_REQUIRE(Q >= 1 && k >= 1 && G >= 1 && n >= 1 && n <= 8, "distinct_class_topn: bad shape (n must be 1..8)");
    hipLaunchKernelGGL(k_distinct_topn, dim3((unsigned)cdiv(Q, 128)), dim3(128), 0, (hipStream_t)stream,
                       (const i64*)idx, val, (i64)Q, k, (const i64*)gallery_cls, (i64)G, n, (i64*)out_cls, (i64*)out_idx,
                       out_val);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
