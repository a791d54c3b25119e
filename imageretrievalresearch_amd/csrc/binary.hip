// Binary (sign-bit) resident gallery: a row is dim bits, bit j set iff n[j] >= center[j] for the normalised row n, and the score
// of a pair is the cosine of the two +-1 vectors, (dim - 2 * popcount(q xor g)) / dim.  The format is specified bit for bit in
// include/mi355_retrieval.h (integer arithmetic and one fp32 division: no tolerance anywhere).
//   k_bin_encode ... one wave per row: the row's norm as mi355_l2_normalize_rows takes it (row_inv_norm), x * r against the
//                    centre, 64 dimensions per ballot = two code words; pad words zeroed; for queries a NaN flag per row
//   k_bin_scan ..... one workgroup per (chunk of 256 rows, block of 64 queries).  The chunk's code rows come from memory with
//                    coalesced 16-byte loads into LDS (row stride S + 1 words: odd, so the 32 lanes of a read hit 32 banks),
//                    then every lane holds ONE row in S registers.  A query's words are the same for the whole wave: they are
//                    read through uniform addresses (scalar loads), so a lane's inner loop is xor + accumulating popcount per
//                    word, and the row in registers is reused by every query of the block.  Two endings:
//                      DIST .... the distances h as int32 (mi355_binary_distances)
//                      FUSED ... per pass of 32 queries the keys (h << 8 | row in chunk) go to an LDS tile, eight threads per
//                                query keep the K smallest of 32 keys each in a branch-free sorted list and merge them by a
//                                butterfly of shuffles; a smaller key IS a better candidate (lower distance, then the lower
//                                row), so ties need no rule of their own.  K candidates per (query, chunk) leave the CU.
//                    Rows longer than S = 48 words (dim > 1536) are taken in slices of 48 words, the partial distances kept
//                    in the LDS tile (MULTI).
//   k > 8 .......... no score slab: the scan leaves each chunk's 8 best rows (C).  Let b be the k-th best of C.  A row of the
//                    top-k that is not in C lies in a chunk whose 8 candidates all beat it, so that chunk's 8th candidate is
//                    not worse than b - a SATURATED chunk - and since only k candidates are not worse than b, a query has at
//                    most k / 8 of them.  k_bin_saturated lists them in chunk order and retires their candidates,
//                    k_bin_rescan scores every row of those chunks for that query, and the selection over both is exact.
//   asymmetric ..... the same codes searched with int8 query codes on the i8 MFMA (k_bin_asym_queries, k_bin_asym_scan: see
//                    the block in front of them); staging, selection pass and the k > 8 route are shared with the above.
// No atomics: every output slot has one writer.  gfx950 only.
#include "i8_quant.h"
#include "../../include/mi355_retrieval.h"

#include <type_traits>

namespace mi355 {

constexpr int BIN_MAX_DIM = 65536;
constexpr int BIN_CHUNK = 256;                 // rows of one scan workgroup: one per thread
constexpr int BIN_QB = 64;                     // queries of one scan workgroup: the reuse of a row in registers
constexpr int BIN_QP = 32;                     // queries of one pass of the fused selection: eight threads per query
constexpr int BIN_TS = 8 * 33 + 1;             // words of one query's keys in the tile: thread t at (t / 32) * 33 + t % 32
constexpr int BIN_SLICE = 48;                  // the most words of a row a lane holds: 1536 bits
constexpr i64 BIN_QBLOCK = 256;                // queries of one scan launch
constexpr i64 BIN_CAND_ELEMS = (i64)1 << 26;   // candidates of one query block (k > 8): 12 bytes each, under 768 MB
constexpr unsigned BIN_NO_KEY = 0xffffffffu;   // an ineligible or missing row: above every real key
enum { BIN_DIST = 0, BIN_FUSED = 2 };

__host__ __device__ __forceinline__ int bin_words(int dim) { return (dim + 31) / 32; }
__host__ __device__ __forceinline__ int bin_ld(int dim) { return (bin_words(dim) + 3) & ~3; }
// The words of a row one lane holds at a time, and the stride of the query codes in the workspace: whole slices, pad words 0
static int bin_slice(int ld) { return ld <= 4 ? 4 : ld <= 16 ? 16 : BIN_SLICE; }
static int bin_ldq(int ld) { const int s = bin_slice(ld); return (ld + s - 1) / s * s; }

// score = float(dim - 2 h) / float(dim): both conversions exact (|dim - 2 h| <= 65536), one IEEE division
__device__ __forceinline__ float bin_score(int h, int dim) { return __fdiv_rn((float)(dim - 2 * h), (float)dim); }

// ---- encode: wave w of workgroup b takes rows b * 4 + w, + 4 * gridDim.x, ...; codes [R][ld_out] words, ld_out even
template <bool NORM>
__global__ __launch_bounds__(256) void k_bin_encode(const float* __restrict__ rows, const float* __restrict__ center,
                                                    unsigned* __restrict__ codes, int* __restrict__ nanflag, i64 R, int dim,
                                                    int ld_out, float eps, int vec) {
    const int lane = threadIdx.x & 63;
    for (i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (i64)gridDim.x * 4) {
        const float* x = rows + row * dim;
        const float r = NORM ? row_inv_norm(x, dim, eps, vec, lane) : 1.0f;
        uint2* out = reinterpret_cast<uint2*>(codes + row * ld_out);
        bool bad = false;
        for (int p = 0; p < ld_out / 2; ++p) {
            const int j = p * 64 + lane;
            bool bit = false;
            if (j < dim) {
                const float v = NORM ? x[j] * r : x[j];
                bit = v >= (center ? center[j] : 0.0f);                // a NaN on either side: false
                bad = bad || v != v;
            }
            const unsigned long long b = __ballot(bit);                 // bit `lane` = dimension j: word j / 32, position j % 32
            if (lane == 0) out[p] = make_uint2((unsigned)b, (unsigned)(b >> 32));
        }
        if (nanflag) {
            const int any = __any(bad);
            if (lane == 0) nanflag[row] = any;
        }
    }
}

// ---- scan
struct BinScanArgs {
    const unsigned* codes;      // [G][ld]
    i64 G;
    int ld;
    const unsigned* qcodes;     // [Q][ldq] the codes of this launch's queries
    const int* qnan;            // [Q] 1: the query's normalised row holds a NaN
    int Q, ldq, dim, k, nch;
    i64 idx_offset;
    int* out;                   // DIST: distances [Q][ld_out]
    i64 ld_out;
    float* cand_val;            // FUSED: [Q][cand_ld], chunk c at c * k
    i64* cand_idx;
    i64 cand_ld;
    RankFilter flt;             // FUSED && FILT: the filter of this launch's queries
};

// Words [s0, s0 + S) of the chunk's 256 rows into rows_s [256][S + 1]; a row past G or a word past ld reads as 0.  (S is a
// constant of the popcount scan and a launch-wide value of the asymmetric one: inlined, the former compiles as before.)
__device__ __forceinline__ void bin_stage_words(unsigned* rows_s, const BinScanArgs& a, i64 c0, int s0, const int S) {
    const int PPR = S / 4;                                              // 16-byte pieces of a row slice
    for (int p = threadIdx.x; p < BIN_CHUNK * PPR; p += 256) {
        const int row = p / PPR, w0 = s0 + (p - row * PPR) * 4;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c0 + row < a.G && w0 < a.ld) v = *reinterpret_cast<const uint4*>(a.codes + (c0 + row) * a.ld + w0);
        unsigned* d = rows_s + row * (S + 1) + (w0 - s0);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}
template <int S>
__device__ __forceinline__ void bin_stage(unsigned* rows_s, const BinScanArgs& a, i64 c0, int s0) {
    bin_stage_words(rows_s, a, c0, s0, S);
}

// The ending of one pass of the fused scans.  tile [BIN_QP][BIN_TS] holds the pass's keys (distance << 8 | row in chunk,
// BIN_NO_KEY for an ineligible row), query qq of the pass is query q0 + qq of the launch and takes part iff q_lo <= q0 + qq <
// q_hi.  Thread t: query t / 8 of the pass, keys part * 33 .. part * 33 + 31 of it (rows part * 32 .. + 31 of the chunk): it
// keeps the K smallest in a branch-free sorted list, the eight lists of a query are merged by a butterfly of shuffles, and
// part 0 writes the a.k best as (score(q)(distance), row) to the chunk's candidate slots.  No barrier inside.
template <int K, class Score>
__device__ __forceinline__ void bin_select_pass(const unsigned* tile, const BinScanArgs& a, int chunk, i64 c0, int q0, int q_lo, int q_hi,
                                                const Score& score) {
    const int tid = threadIdx.x;
    const int qq = tid >> 3, part = tid & 7;
    const int q = q0 + qq;
    const bool mine_q = q >= q_lo && q < q_hi;                          // (whole groups of 8 lanes: the shuffles below stay inside one)
    unsigned kv[K];
#pragma unroll
    for (int i = 0; i < K; ++i) kv[i] = BIN_NO_KEY;
    auto insert = [&](unsigned key) {                                   // keys are distinct; BIN_NO_KEY is below nothing
        bool g[K];
#pragma unroll
        for (int i = 0; i < K; ++i) g[i] = key < kv[i];
#pragma unroll
        for (int i = K - 1; i > 0; --i) kv[i] = g[i] ? (g[i - 1] ? kv[i - 1] : key) : kv[i];
        kv[0] = g[0] ? key : kv[0];
    };
    if (mine_q) {
        const unsigned* mine = tile + qq * BIN_TS + part * 33;
#pragma unroll 4
        for (int i = 0; i < 32; ++i) insert(mine[i]);
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        unsigned other[K];
#pragma unroll
        for (int i = 0; i < K; ++i) other[i] = (unsigned)__shfl_xor((int)kv[i], m, 64);
#pragma unroll
        for (int i = 0; i < K; ++i) insert(other[i]);
    }
    if (part == 0 && mine_q) {
        const size_t o = (size_t)q * a.cand_ld + (size_t)chunk * a.k;
        const auto score_of = score(q);                                 // the query's constants, read once
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i < a.k) {
                const bool have = kv[i] != BIN_NO_KEY;
                a.cand_val[o + i] = have ? score_of((int)(kv[i] >> 8)) : NEG_INF;
                a.cand_idx[o + i] = have ? c0 + (i64)(kv[i] & 255u) + a.idx_offset : IDX_PAD;
            }
        }
    }
}

// grid: cdiv(Q, BIN_QB) query blocks (fastest) x nch chunks, one-dimensional
template <int S, int MODE, int K, bool FILT, bool MULTI>
__global__ __launch_bounds__(256) void k_bin_scan(BinScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned smem[];
    unsigned* rows_s = smem;                                            // [256][S + 1]
    // the pass's keys or partial distances [BIN_QP][BIN_TS]; without slices the rows are in registers by then: the same LDS
    unsigned* tile = MULTI ? smem + BIN_CHUNK * (S + 1) : smem;
    const int tid = threadIdx.x;
    const int nqb = (a.Q + BIN_QB - 1) / BIN_QB;
    const int chunk = blockIdx.x / nqb, qblk = blockIdx.x - chunk * nqb;
    const i64 c0 = (i64)chunk * BIN_CHUNK, row = c0 + tid;
    const bool live = row < a.G;
    const int q_lo = qblk * BIN_QB, q_hi = q_lo + BIN_QB < a.Q ? q_lo + BIN_QB : a.Q;
    const int slot = (tid >> 5) * 33 + (tid & 31);
    i64 glab = 0;
    if constexpr (MODE == BIN_FUSED && FILT) {
        if (live && a.flt.mode != MI355_LABEL_ANY) glab = a.flt.glab[row];
    }
    unsigned r[S];
    auto load_row = [&]() {
#pragma unroll
        for (int w = 0; w < S; ++w) r[w] = rows_s[tid * (S + 1) + w];
    };
    auto partial = [&](int q, int s0) {
        const unsigned* __restrict__ qw = a.qcodes + (size_t)q * a.ldq + s0;       // the same address in every lane
        // two chains of xor + accumulating popcount (v_bcnt_u32_b32 adds its third operand).  The empty asm keeps each running
        // sum in one register: left alone the compiler rebalances the sum into popcounts of 0 and three-way adds, 2.5
        // instructions per word for 2.  It emits nothing.
        int h0 = 0, h1 = 0;
#pragma unroll
        for (int w = 0; w < S; w += 2) {
            h0 += __popc(r[w] ^ qw[w]);
            asm("" : "+v"(h0));
            h1 += __popc(r[w + 1] ^ qw[w + 1]);
            asm("" : "+v"(h1));
        }
        return h0 + h1;
    };
    if constexpr (!MULTI) {
        bin_stage<S>(rows_s, a, c0, 0);
        __syncthreads();
        load_row();
        __syncthreads();                                                // the tile may take the rows' place now
    }
    for (int qp = q_lo; qp < q_hi; qp += BIN_QP) {
        const int nq = q_hi - qp < BIN_QP ? q_hi - qp : BIN_QP;
        if constexpr (MULTI) {
            for (int s0 = 0; s0 < a.ld; s0 += S) {
                __syncthreads();                                        // every lane has left the previous slice (and tile)
                bin_stage<S>(rows_s, a, c0, s0);
                __syncthreads();
                load_row();
                for (int qq = 0; qq < nq; ++qq) {                       // a thread's own slots: no barrier
                    const int h = partial(qp + qq, s0);
                    tile[qq * BIN_TS + slot] = s0 ? tile[qq * BIN_TS + slot] + (unsigned)h : (unsigned)h;
                }
            }
        }
        for (int qq = 0; qq < nq; ++qq) {
            const int q = qp + qq;
            const int h = MULTI ? (int)tile[qq * BIN_TS + slot] : partial(q, 0);
            const bool qbad = a.qnan[q] != 0;
            if constexpr (MODE == BIN_DIST) {
                if (live) a.out[(i64)q * a.ld_out + row] = qbad ? -1 : h;
            } else {
                bool ok = live;
                if constexpr (FILT) {
                    i64 fq_lab, fq_ex;
                    query_filter(a.flt, q, fq_lab, fq_ex);
                    ok = ok && eligible(a.flt.mode, fq_lab, glab, fq_ex, row);
                }
                // a NaN query scores NaN everywhere: all tie, the lower row first
                tile[qq * BIN_TS + slot] = ok ? ((unsigned)(qbad ? 0 : h) << 8) | (unsigned)tid : BIN_NO_KEY;
            }
        }
        if constexpr (MODE == BIN_FUSED) {
            __syncthreads();
            bin_select_pass<K>(tile, a, chunk, c0, qp, q_lo, q_hi, [&](int q) {
                const bool qbad = a.qnan[q] != 0;
                const int dim = a.dim;
                return [=](int h) { return qbad ? __uint_as_float(0x7fc00000u) : bin_score(h, dim); };
            });
            __syncthreads();                                            // the next pass writes the tile
        }
    }
}

// ---- asymmetric scoring: the gallery stays bits, the query becomes int8 codes u of r = n - center (the row quantiser of
// i8_quant.h), and the distance is the Hamming distance weighted by |u|: m = Upos - P with P = the sum of u over the set bits of
// the row and Upos = the sum of the positive u.  P is an int8 dot product of u with the row's bits as 0/1 bytes, so it runs on
// v_mfma_i32_32x32x32_i8 with exact int32 sums.  score = float(L1 - 2 m) / float(L1), L1 = sum |u|.
//   k_bin_asym_queries ... one wave per query: norm, r, amax, the codes in the order the scan's A fragments want them
//   k_bin_asym_scan ...... one workgroup per (chunk of 256 rows, block of 64 queries); a wave takes 64 rows of the chunk as two
//                          B tiles of 32 columns and the block's queries as one or two A tiles of 32 rows.  Per k-step of 32
//                          dimensions a lane reads one word of each of its two rows from the LDS image, expands its 16 bits
//                          to 16 bytes of 0 / 1 ((nibble * 0x00204081) & 0x01010101: bit i of the nibble lands in byte i) and
//                          issues 2 x tiles MFMAs.  A lane's A and B bytes are the same 16 dimensions, byte for byte, and an
//                          integer sum has no order (the pairing argument of rank_i8.hip).  The endings are those of k_bin_scan.
// Queries of one asymmetric scan workgroup: two A tiles, 64 accumulator registers per lane.  Measured at 1M rows x 1536
// (plain k = 3, Q = 256 / Q = 1): 128 queries at one wave per SIMD 1.35 / 0.29 ms, held to two waves (it spills) 1.31 / 0.24,
// 64 queries at two waves 0.91 / 0.19, at three waves 0.85 / 0.17 - the bits are expanded twice as often, but the loop is
// bound by the latency of its loads, and the waves hide it.
constexpr int BIN_AQB = 64;
constexpr int BIN_ANT = BIN_AQB / 32;
constexpr int BIN_ASYM_WGS = 3;                // workgroups per CU the scan is compiled for: at most 170 VGPRs
static_assert(BIN_ANT == 2, "k_bin_asym_scan has a k-loop for one live tile and one for both");
typedef int bin_i32x16 __attribute__((ext_vector_type(16)));

// The queries of an asymmetric call.  frag [tile of 32 queries][k-step][lane][16 B]: lane = query % 32 + 32 * half holds the
// codes of dimensions step * 32 + half * 16 .. + 15; whole tiles, the rows past Q and the dimensions past dim are 0.
struct BinAsymQueries {
    const signed char* frag;
    const int* upos;            // [Q up to whole tiles] the sum of the positive codes
    const int* l1;              // the sum of |code|
    const int* qnan;            // 1: a NaN in r, or a non-finite amax
    int steps;                  // ceil(dim / 32)
    // float(L1 - 2 m) / float(L1): both conversions exact (|L1 - 2 m| <= L1 < 2^23), one IEEE division
    // (score_of(q): the query's two integers read once, then a function of m)
    __device__ __forceinline__ auto score_of(int q) const {
        const bool bad = qnan[q] != 0;
        const int L = l1[q];
        return [=](int m) {
            if (bad) return __uint_as_float(0x7fc00000u);
            return L == 0 ? 0.0f : __fdiv_rn((float)(L - 2 * m), (float)L);
        };
    }
    __device__ __forceinline__ float score(int q, int m) const { return score_of(q)(m); }
};

// bits 0 .. 3 of nib as four bytes of 0 / 1
__device__ __forceinline__ unsigned bin_expand4(unsigned nib) { return (nib * 0x00204081u) & 0x01010101u; }
__device__ __forceinline__ i32x4 bin_expand16(unsigned bits) {
    return (i32x4){(int)bin_expand4(bits & 15u), (int)bin_expand4((bits >> 4) & 15u), (int)bin_expand4((bits >> 8) & 15u),
                   (int)bin_expand4((bits >> 12) & 15u)};
}

// P of (query q, the code row g) on the VALU: for the rescan of the saturated chunks
__device__ __forceinline__ int bin_asym_row_sum(const BinAsymQueries& aq, int q, const unsigned* __restrict__ g) {
    const signed char* f = aq.frag + (size_t)(q >> 5) * aq.steps * 1024 + (q & 31) * 16;
    int p = 0;
    for (int w = 0; w < aq.steps; ++w) {
        const unsigned bits = g[w];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const i32x4 u = *reinterpret_cast<const i32x4*>(f + (size_t)w * 1024 + h * 512);
            const i32x4 b = bin_expand16(bits >> (16 * h));
#pragma unroll
            for (int e = 0; e < 4; ++e) p = __builtin_amdgcn_sdot4(u[e], b[e], p, false);
        }
    }
    return p;
}

// wave w of workgroup b takes row b * 4 + w of the rows_pad rows; rows >= Q (the rest of the last tile) are written as zeros.
// frag, upos null: only plain [Q][dim], l1 and qnan are written (mi355_binary_asym_query_codes); plain null otherwise.
__global__ __launch_bounds__(256) void k_bin_asym_queries(const float* __restrict__ queries, const float* __restrict__ center, int Q,
                                                          int rows_pad, int dim, float eps, int vec, signed char* __restrict__ frag,
                                                          int steps, int* __restrict__ upos, int* __restrict__ l1,
                                                          int* __restrict__ qnan, signed char* __restrict__ plain) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_pad) return;
    signed char* out = frag ? frag + (size_t)(row >> 5) * steps * 1024 + (row & 31) * 16 : nullptr;
    const bool real = row < Q;
    const float* x = queries + (i64)(real ? row : 0) * dim;
    I8Quant q = {0.f, 0.f, true};
    float r = 0.f;
    if (real) {
        r = row_inv_norm(x, dim, eps, vec, lane);
        float amax = 0.f;
        bool nan = false;
        for (int i = lane; i < dim; i += 64) {
            const float d = i8_norm_elem(x[i], r) - (center ? center[i] : 0.0f);
            nan = nan || d != d;
            amax = fmaxf(amax, fabsf(d));
        }
        q = i8_quant(wave_max(amax), __ballot(nan) != 0ull);
    }
    int sum_abs = 0, sum_pos = 0;
    for (int c = lane; c < 2 * steps; c += 64) {                        // 16-byte piece c: k-step c / 2, half c % 2
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (!q.zero) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = c * 16 + j;
                int u = 0;
                if (k < dim) u = i8_code(i8_norm_elem(x[k], r) - (center ? center[k] : 0.0f), q.inv);
                sum_abs += u < 0 ? -u : u;
                sum_pos += u > 0 ? u : 0;
                w[j >> 2] |= (unsigned)(u & 0xff) << (8 * (j & 3));
            }
        }
        if (out) *reinterpret_cast<i32x4*>(out + (size_t)(c >> 1) * 1024 + (c & 1) * 512) = (i32x4){(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
        if (plain && real) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = c * 16 + j;
                if (k < dim) plain[(i64)row * dim + k] = (signed char)((w[j >> 2] >> (8 * (j & 3))) & 0xff);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum_abs += __shfl_xor(sum_abs, o, 64); sum_pos += __shfl_xor(sum_pos, o, 64); }
    if (lane == 0) {
        l1[row] = sum_abs;
        qnan[row] = q.zero && q.scale != q.scale ? 1 : 0;
        if (upos) upos[row] = sum_pos;
    }
}

struct BinAsymScanArgs {
    BinScanArgs s;              // codes, G, ld, Q = the queries of this launch, k, nch, the outputs and the filter; no qcodes
    BinAsymQueries aq;          // the queries of the call
    int aq0;                    // query q of the launch is query aq0 + q of the call
    int S;                      // words of a row in the LDS image at a time: min(ld, BIN_SLICE)
};

// grid: query blocks (fastest) x nch chunks, one-dimensional.  The A tiles are tiles of 32 of the CALL's queries; a launch's
// queries aq0 .. aq0 + Q - 1 may start and end inside one (aq0 need not be a multiple of 32: the query block of k > 8 over a
// very large gallery is whatever fits the candidate lists).  The launch covers every tile it touches, a workgroup takes up to
// BIN_ANT consecutive ones, computes all 32 rows of each and leaves out the queries of another launch (q < 0 or q >= Q below).
template <int MODE, int K, bool FILT>
__global__ __launch_bounds__(256, BIN_ASYM_WGS) void k_bin_asym_scan(BinAsymScanArgs b) {
    extern __shared__ __attribute__((aligned(16))) unsigned smem[];
    unsigned* rows_s = smem;                                            // [256][S + 1]
    unsigned* tile = smem;                                              // the keys of a pass, once the k-loop has left the rows
    const BinScanArgs& a = b.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int t_first = b.aq0 >> 5, t_end = (b.aq0 + a.Q + 31) >> 5;
    const int nqb = (t_end - t_first + BIN_ANT - 1) / BIN_ANT;
    const int chunk = blockIdx.x / nqb, qblk = blockIdx.x - chunk * nqb;
    const int t0 = t_first + qblk * BIN_ANT;
    const int nt = t_end - t0 < BIN_ANT ? t_end - t0 : BIN_ANT;         // live tiles: the same in every thread
    const i64 c0 = (i64)chunk * BIN_CHUNK;
    const int steps = b.aq.steps, S = b.S;
    bin_i32x16 acc[2][BIN_ANT];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < BIN_ANT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][t][r] = 0;
    const unsigned* my0 = rows_s + (wave * 64 + col) * (S + 1);
    const unsigned* my1 = my0 + 32 * (S + 1);
    for (int s0 = 0; s0 < steps; s0 += S) {
        __syncthreads();                                                // every lane has left the previous slice
        bin_stage_words(rows_s, a, c0, s0, S);
        __syncthreads();
        const int nw = steps - s0 < S ? steps - s0 : S;
        const signed char* fa = b.aq.frag + ((size_t)t0 * steps + s0) * 1024 + lane * 16;
        auto k_loop = [&](auto live_tiles) {                            // (a branch-free body per number of live tiles)
            constexpr int NTL = decltype(live_tiles)::value;
            for (int w = 0; w < nw; ++w) {
                const i32x4 b0 = bin_expand16(my0[w] >> (16 * half)), b1 = bin_expand16(my1[w] >> (16 * half));
#pragma unroll
                for (int t = 0; t < NTL; ++t) {
                    const i32x4 af = *reinterpret_cast<const i32x4*>(fa + ((size_t)t * steps + w) * 1024);
                    acc[0][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, b0, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, b1, acc[1][t], 0, 0, 0);
                }
            }
        };
        if (nt == 1) k_loop(std::integral_constant<int, 1>{});
        else k_loop(std::integral_constant<int, BIN_ANT>{});
    }
    // accumulator register r of a lane: query (r & 3) + 8 * (r >> 2) + 4 * half of the tile, row col (+ 32) of the wave's 64
    const int rc[2] = {wave * 64 + col, wave * 64 + 32 + col};
    const bool live[2] = {c0 + rc[0] < a.G, c0 + rc[1] < a.G};
    i64 glab[2] = {0, 0};
    if constexpr (MODE == BIN_FUSED && FILT) {
        if (a.flt.mode != MI355_LABEL_ANY) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (live[j]) glab[j] = a.flt.glab[c0 + rc[j]];
        }
    }
    if constexpr (MODE == BIN_FUSED) __syncthreads();                   // the tile takes the rows' place
#pragma unroll
    for (int t = 0; t < BIN_ANT; ++t) {
        if (t < nt) {
            const int qt = (t0 + t) * 32;                               // the tile's first query, of the call
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int q = qt + qq - b.aq0;                          // of the launch
                const bool mine_q = q >= 0 && q < a.Q;
                const int up = b.aq.upos[qt + qq];
                const bool qbad = b.aq.qnan[qt + qq] != 0;
                i64 fq_lab = 0, fq_ex = -1;
                if constexpr (MODE == BIN_FUSED && FILT) {
                    if (mine_q) query_filter(a.flt, q, fq_lab, fq_ex);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int m = up - acc[j][t][r];
                    if constexpr (MODE == BIN_DIST) {
                        if (mine_q && live[j]) a.out[(i64)q * a.ld_out + c0 + rc[j]] = qbad ? -1 : m;
                    } else {
                        bool ok = live[j];
                        if constexpr (FILT) ok = ok && eligible(a.flt.mode, fq_lab, glab[j], fq_ex, c0 + rc[j]);
                        // m < 2^23: the key stays below BIN_NO_KEY.  A NaN query scores NaN everywhere: all tie
                        tile[qq * BIN_TS + (rc[j] >> 5) * 33 + (rc[j] & 31)] =
                            ok ? ((unsigned)(qbad ? 0 : m) << 8) | (unsigned)rc[j] : BIN_NO_KEY;
                    }
                }
            }
            if constexpr (MODE == BIN_FUSED) {
                __syncthreads();
                bin_select_pass<K>(tile, a, chunk, c0, qt - b.aq0, 0, a.Q, [&](int q) { return b.aq.score_of(b.aq0 + q); });
                __syncthreads();                                        // the next pass writes the tile
            }
        }
    }
}

// ---- k > 8: the saturated chunks of each query.  grid (queries), 256 threads.  A query's candidates are cand [cand_ld]: chunk c
// at c * 8, best first, missing ones (fewer than 8 eligible rows) as pads at the end.  bound_val / bound_idx [queries][k]: the
// k best candidates in order (null: fewer than k candidates exist at all, so there is no bound); a pad in slot k - 1 (-1 after a
// filtered selection, IDX_PAD otherwise) means the same.  Chunk c is saturated iff it has 8 candidates and the bound does not
// beat its 8th.  Their ids go to satlist [queries][nslots] in ascending order (a prefix over the threads: no atomics), their
// number to satcount, and their 8 candidates are retired: k_bin_rescan brings every row of the chunk back.
__global__ __launch_bounds__(256) void k_bin_saturated(const float* __restrict__ cand_val, i64* __restrict__ cand_idx, i64 cand_ld, int nch,
                                                       const float* __restrict__ bound_val, const i64* __restrict__ bound_idx, int k,
                                                       int nslots, int* __restrict__ satlist, int* __restrict__ satcount) {
    __shared__ int wave_cnt[4];
    const i64 q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* cv = cand_val + q * cand_ld;
    i64* ci = cand_idx + q * cand_ld;
    float bv = 0.f;
    i64 bi = -1;
    if (bound_idx) { bv = bound_val[q * k + k - 1]; bi = bound_idx[q * k + k - 1]; }
    const bool has_bound = bi >= 0 && bi < NO_CAND_IDX;
    int total = 0;                                                      // saturated chunks before this trip (uniform)
    for (int c0 = 0; c0 < nch; c0 += 256) {
        const int c = c0 + tid;
        bool sat = false;
        if (c < nch) {
            const i64 wi = ci[(i64)c * 8 + 7];
            sat = wi < NO_CAND_IDX && !(has_bound && better(bv, bi, cv[(i64)c * 8 + 7], wi));
        }
        const unsigned long long m = __ballot(sat);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int pos = total + __popcll(m & ((1ull << lane) - 1));
        int trip = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) pos += wave_cnt[w];
            trip += wave_cnt[w];
        }
        if (sat) {
            if (pos < nslots) satlist[q * nslots + pos] = c;             // (at most k / 8 = nslots of them: see the file's head)
#pragma unroll
            for (int i = 0; i < 8; ++i) ci[(i64)c * 8 + i] = IDX_PAD;
        }
        total += trip;
        __syncthreads();                                                // wave_cnt is rewritten by the next trip
    }
    if (tid == 0) satcount[q] = total < nslots ? total : nslots;
}

// ---- k > 8: every row of the saturated chunks.  grid (nslots, queries), thread = row of the chunk; slot s of query q writes
// cand [q][tail + s * 256 + tid], a pad where the slot is unused, the row is past G or the filter rejects it.  A lane reads its
// own code row here (uncoalesced): at most k / 8 chunks per query, a thousandth of the scan's bytes.
struct BinRescanArgs {
    const unsigned* codes; i64 G; int ld;
    const unsigned* qcodes; const int* qnan; int ldq, dim, nslots;
    const int* satlist; const int* satcount;
    i64 idx_offset, cand_ld, tail;
    float* cand_val; i64* cand_idx;
    RankFilter flt; int filt;
    BinAsymQueries aq; int aq0;     // ASYM: the queries' int8 codes; query q of the launch is query aq0 + q of them
};
template <bool ASYM>
__global__ __launch_bounds__(256) void k_bin_rescan(BinRescanArgs a) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const i64 q = blockIdx.y;
    const size_t o = (size_t)q * a.cand_ld + a.tail + (size_t)s * BIN_CHUNK + tid;
    float val = NEG_INF;
    i64 idx = IDX_PAD;
    if (s < a.satcount[q]) {
        const i64 row = (i64)a.satlist[q * a.nslots + s] * BIN_CHUNK + tid;
        bool ok = row < a.G;
        if (ok && a.filt) {
            i64 fq_lab, fq_ex;
            query_filter(a.flt, q, fq_lab, fq_ex);
            ok = eligible(a.flt.mode, fq_lab, a.flt.mode != MI355_LABEL_ANY ? a.flt.glab[row] : 0, fq_ex, row);
        }
        if (ok) {
            const unsigned* g = a.codes + row * a.ld;
            if constexpr (ASYM) {
                const int qa = a.aq0 + (int)q;
                val = a.aq.score(qa, a.aq.upos[qa] - bin_asym_row_sum(a.aq, qa, g));
            } else {
                const unsigned* qw = a.qcodes + q * a.ldq;
                int h = 0;
                for (int w = 0; w < a.ld; ++w) h += __popc(g[w] ^ qw[w]);
                val = a.qnan[q] ? __uint_as_float(0x7fc00000u) : bin_score(h, a.dim);
            }
            idx = row + a.idx_offset;
        }
    }
    a.cand_val[o] = val;
    a.cand_idx[o] = idx;
}

// ---- host side
struct BinWs {
    unsigned* qcodes; int* qnan; float* cand_val; i64* cand_idx; int* satlist; int* satcount; void* topk; size_t topk_bytes;
    size_t total;
};
// Candidates of one query: k per chunk (k <= 8), or 8 per chunk and behind them 256 per saturated chunk, k / 8 at most (k > 8)
static i64 bin_cand_ld(i64 G, int k) {
    const i64 nch = (G + BIN_CHUNK - 1) / BIN_CHUNK;
    return k <= SMALL_K ? nch * k : nch * SMALL_K + (i64)(k / SMALL_K) * BIN_CHUNK;
}
static i64 bin_query_block(i64 Q, i64 G, int k) {
    i64 qb = BIN_QBLOCK;
    if (k > SMALL_K) {
        const i64 fit = BIN_CAND_ELEMS / bin_cand_ld(G, k);
        if (fit < qb) qb = fit < 1 ? 1 : fit;
    }
    return qb < Q ? qb : Q;
}
// Scratch of a search over Q queries (k = 0: mi355_binary_distances, no selection): the queries' codes and NaN flags, then a
// query block's candidate lists, for k > 8 its saturated chunks, and the selection's own scratch
static BinWs bin_carve(void* ws, i64 Q, i64 G, int dim, int k) {
    BinWs r{};
    WsCarver c(ws);
    const i64 qb = bin_query_block(Q, G, k);
    r.qcodes = (unsigned*)c.take((size_t)Q * bin_ldq(bin_ld(dim)) * sizeof(unsigned));
    r.qnan = (int*)c.take((size_t)Q * sizeof(int));
    if (k >= 1) {
        const size_t n = (size_t)qb * bin_cand_ld(G, k);
        r.cand_val = (float*)c.take(n * sizeof(float));
        r.cand_idx = (i64*)c.take(n * sizeof(i64));
        if (k > SMALL_K) {
            r.satlist = (int*)c.take((size_t)qb * (k / SMALL_K) * sizeof(int));
            r.satcount = (int*)c.take((size_t)qb * sizeof(int));
        }
        r.topk_bytes = topk_ws_bytes(qb, bin_cand_ld(G, k), k);         // (both selections of k > 8: the longer row)
        r.topk = c.take(r.topk_bytes);
    }
    r.total = c.total();
    return r;
}

static bool bin_shape_ok(i64 Q, i64 G, int dim) {
    return Q >= 0 && G >= 0 && dim >= 1 && dim <= BIN_MAX_DIM && Q <= INT_MAX && G <= (i64)INT_MAX;
}

static int launch_encode(const float* rows, i64 R, int dim, int normalized, float eps, const float* center, unsigned* codes, int ld_out,
                         int* nanflag, hipStream_t st) {
    const i64 want = (R + 3) / 4;
    const dim3 grid((unsigned)(want < ((i64)1 << 22) ? want : ((i64)1 << 22)));
    if (normalized) hipLaunchKernelGGL(k_bin_encode<false>, grid, dim3(256), 0, st, rows, center, codes, nanflag, R, dim, ld_out, eps, 0);
    else hipLaunchKernelGGL(k_bin_encode<true>, grid, dim3(256), 0, st, rows, center, codes, nanflag, R, dim, ld_out, eps, vec_ok(rows, dim));
    MI355_LAUNCH_CHECK();
    return OK;
}

template <int S, int MODE, int K, bool FILT, bool MULTI>
static int launch_scan(const BinScanArgs& a, hipStream_t st) {
    constexpr size_t rows_b = (size_t)BIN_CHUNK * (S + 1) * sizeof(unsigned), tile_b = (size_t)BIN_QP * BIN_TS * sizeof(unsigned);
    constexpr size_t lds = MULTI ? rows_b + tile_b : (MODE == BIN_FUSED && tile_b > rows_b ? tile_b : rows_b);
    if constexpr (lds > 64 * 1024) {                                    // (the sliced scan: rows and tile side by side)
        static bool done[MI355_MAX_DEVICES] = {false};
        if (first_time_on_this_device(done))
            MI355_CHECK_HIP(hipFuncSetAttribute((const void*)k_bin_scan<S, MODE, K, FILT, MULTI>,
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    const unsigned grid = (unsigned)a.nch * (unsigned)((a.Q + BIN_QB - 1) / BIN_QB);
    hipLaunchKernelGGL((k_bin_scan<S, MODE, K, FILT, MULTI>), dim3(grid), dim3(256), lds, st, a);
    MI355_LAUNCH_CHECK();
    return OK;
}
template <int MODE, int K, bool FILT>
static int dispatch_slice(const BinScanArgs& a, hipStream_t st) {
    if (a.ld <= 4) return launch_scan<4, MODE, K, FILT, false>(a, st);
    if (a.ld <= 16) return launch_scan<16, MODE, K, FILT, false>(a, st);
    if (a.ld <= BIN_SLICE) return launch_scan<BIN_SLICE, MODE, K, FILT, false>(a, st);
    return launch_scan<BIN_SLICE, MODE, K, FILT, true>(a, st);
}
template <bool FILT>
static int dispatch_fused(const BinScanArgs& a, hipStream_t st) {
    if (a.k <= 1) return dispatch_slice<BIN_FUSED, 1, FILT>(a, st);
    if (a.k <= 4) return dispatch_slice<BIN_FUSED, 4, FILT>(a, st);
    return dispatch_slice<BIN_FUSED, 8, FILT>(a, st);
}

// What mi355_binary_distances and mi355_binary_search check of their common arguments
static int bin_check_search(const char* who, const void* queries, i64 Q, int dim, const void* codes, i64 G, const void* out0,
                            const void* out1) {
    MI355_REQUIRE(queries && codes && out0 && out1, "%s: null pointer", who);
    MI355_REQUIRE(Q >= 0 && G >= 0 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    MI355_REQUIRE(dim <= BIN_MAX_DIM, "%s: dim=%d exceeds %d", who, dim, BIN_MAX_DIM);
    MI355_REQUIRE(((uintptr_t)codes & 15) == 0, "%s: gallery buffer must be 16-byte aligned", who);
    MI355_REQUIRE(Q <= INT_MAX && G <= (i64)INT_MAX, "%s: shape too large Q=%lld G=%lld", who, (long long)Q, (long long)G);
    return OK;
}

// ---- host side of the asymmetric search
struct BinAsymWs {
    signed char* frag; int* upos; int* l1; int* qnan;
    float* cand_val; i64* cand_idx; int* satlist; int* satcount; void* topk; size_t topk_bytes;
    size_t total;
};
// As bin_carve, with the queries' int8 codes (whole tiles of 32 queries) and their three integers in place of the bit codes
static BinAsymWs bin_asym_carve(void* ws, i64 Q, i64 G, int dim, int k) {
    BinAsymWs r{};
    WsCarver c(ws);
    const i64 qb = bin_query_block(Q, G, k), qpad = (Q + 31) / 32 * 32;
    r.frag = (signed char*)c.take((size_t)qpad * bin_words(dim) * 32);
    r.upos = (int*)c.take((size_t)qpad * sizeof(int));
    r.l1 = (int*)c.take((size_t)qpad * sizeof(int));
    r.qnan = (int*)c.take((size_t)qpad * sizeof(int));
    if (k >= 1) {
        const size_t n = (size_t)qb * bin_cand_ld(G, k);
        r.cand_val = (float*)c.take(n * sizeof(float));
        r.cand_idx = (i64*)c.take(n * sizeof(i64));
        if (k > SMALL_K) {
            r.satlist = (int*)c.take((size_t)qb * (k / SMALL_K) * sizeof(int));
            r.satcount = (int*)c.take((size_t)qb * sizeof(int));
        }
        r.topk_bytes = topk_ws_bytes(qb, bin_cand_ld(G, k), k);
        r.topk = c.take(r.topk_bytes);
    }
    r.total = c.total();
    return r;
}

static int launch_asym_queries(const float* queries, i64 Q, i64 rows_pad, int dim, float eps, const float* center, signed char* frag,
                               int* upos, int* l1, int* qnan, signed char* plain, hipStream_t st) {
    hipLaunchKernelGGL(k_bin_asym_queries, dim3((unsigned)((rows_pad + 3) / 4)), dim3(256), 0, st, queries, center, (int)Q, (int)rows_pad,
                       dim, eps, vec_ok(queries, dim), frag, bin_words(dim), upos, l1, qnan, plain);
    MI355_LAUNCH_CHECK();
    return OK;
}
static BinAsymQueries asym_queries(const BinAsymWs& w, int dim) { return {w.frag, w.upos, w.l1, w.qnan, bin_words(dim)}; }

template <int MODE, int K, bool FILT>
static int launch_asym_scan(const BinAsymScanArgs& b, hipStream_t st) {
    const size_t rows_b = (size_t)BIN_CHUNK * (b.S + 1) * sizeof(unsigned), tile_b = (size_t)BIN_QP * BIN_TS * sizeof(unsigned);
    const size_t lds = MODE == BIN_FUSED && tile_b > rows_b ? tile_b : rows_b;              // at most 50176 bytes
    const int tiles = ((b.aq0 + b.s.Q + 31) >> 5) - (b.aq0 >> 5);
    const unsigned grid = (unsigned)b.s.nch * (unsigned)((tiles + BIN_ANT - 1) / BIN_ANT);
    hipLaunchKernelGGL((k_bin_asym_scan<MODE, K, FILT>), dim3(grid), dim3(256), lds, st, b);
    MI355_LAUNCH_CHECK();
    return OK;
}
template <bool FILT>
static int dispatch_asym_fused(const BinAsymScanArgs& b, hipStream_t st) {
    if (b.s.k <= 1) return launch_asym_scan<BIN_FUSED, 1, FILT>(b, st);
    if (b.s.k <= 4) return launch_asym_scan<BIN_FUSED, 4, FILT>(b, st);
    return launch_asym_scan<BIN_FUSED, 8, FILT>(b, st);
}

// The k > 8 route of both searches over one query block, after the scan has left 8 candidates per chunk (cand): the bound into
// (ov, oi), the saturated chunks, their rescan into the tail of cand.  r comes with the queries' side filled in.
template <bool ASYM>
static int bin_saturated_route(BinRescanArgs r, i64 qn, i64 nch, int k, const RankFilter* f, float* ov, i64* oi, int* satlist,
                               int* satcount, void* topk, size_t topk_bytes, hipStream_t st) {
    // the bound: the k-th best of the chunks' candidates, into the output for now (none if there are fewer than k)
    const i64 head = nch * SMALL_K;
    const bool bound = head >= k;
    if (bound)
        if (int e = topk_select(r.cand_val, r.cand_idx, qn, head, r.cand_ld, k, 0, ov, oi, topk, topk_bytes, st, nullptr, f)) return e;
    const int nslots = k / SMALL_K;
    hipLaunchKernelGGL(k_bin_saturated, dim3((unsigned)qn), dim3(256), 0, st, r.cand_val, r.cand_idx, r.cand_ld, (int)nch,
                       bound ? ov : nullptr, bound ? oi : nullptr, k, nslots, satlist, satcount);
    MI355_LAUNCH_CHECK();
    r.nslots = nslots; r.satlist = satlist; r.satcount = satcount; r.tail = head; r.filt = f ? 1 : 0;
    hipLaunchKernelGGL(k_bin_rescan<ASYM>, dim3((unsigned)nslots, (unsigned)qn), dim3(256), 0, st, r);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_binary_bytes(int64_t R, int dim) {
    if (R < 1 || dim < 1 || dim > BIN_MAX_DIM || R > ((int64_t)1 << 40)) return 0;
    return (size_t)R * bin_ld(dim) * sizeof(unsigned);
}

int mi355_binary_encode(const float* rows, int64_t R, int dim, int rows_are_normalized, float eps, const float* center, void* codes,
                        size_t codes_bytes, void* stream) {
    const char* who = "binary_encode";
    MI355_REQUIRE(rows && codes, "%s: null pointer", who);
    MI355_REQUIRE(R >= 0 && dim >= 1, "%s: bad shape R=%lld dim=%d", who, (long long)R, dim);
    MI355_REQUIRE(dim <= BIN_MAX_DIM, "%s: dim=%d exceeds %d", who, dim, BIN_MAX_DIM);
    MI355_REQUIRE(R <= ((int64_t)1 << 40), "%s: shape too large R=%lld", who, (long long)R);
    MI355_REQUIRE(((uintptr_t)codes & 15) == 0, "%s: gallery buffer must be 16-byte aligned", who);
    const size_t need = (size_t)R * bin_ld(dim) * sizeof(unsigned);
    MI355_REQUIRE(codes_bytes >= need, "%s: output buffer %zu < %zu bytes", who, codes_bytes, need);
    if (R == 0) return OK;
    RoctxRange range("binary/encode");
    return launch_encode(rows, R, dim, rows_are_normalized, eps, center, (unsigned*)codes, bin_ld(dim), nullptr, (hipStream_t)stream);
}

size_t mi355_binary_search_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || !bin_shape_ok(Q, G, dim) || k < 0 || k > LARGE_K) return 0;
    return bin_carve(nullptr, Q, G, dim, k).total;
}

int mi355_binary_distances(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G,
                           int32_t* dist, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "binary_distances";
    if (int e = bin_check_search(who, queries, Q, dim, codes, G, dist, dist)) return e;
    if (Q == 0 || G == 0) return OK;
    const BinWs w = bin_carve(workspace, Q, G, dim, 0);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("binary/distances");
    const int ld = bin_ld(dim), ldq = bin_ldq(ld);
    if (int e = launch_encode(queries, Q, dim, 0, eps, center, w.qcodes, ldq, w.qnan, st)) return e;
    const i64 qb = bin_query_block(Q, G, 0), nch = (G + BIN_CHUNK - 1) / BIN_CHUNK;
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = Q - q0 < qb ? Q - q0 : qb;
        BinScanArgs a{};
        a.codes = (const unsigned*)codes; a.G = G; a.ld = ld;
        a.qcodes = w.qcodes + q0 * ldq; a.qnan = w.qnan + q0; a.Q = (int)qn; a.ldq = ldq; a.dim = dim; a.nch = (int)nch;
        a.out = (int*)dist + q0 * G; a.ld_out = G;
        if (int e = dispatch_slice<BIN_DIST, 1, false>(a, st)) return e;
    }
    return OK;
}

int mi355_binary_search(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G, int k,
                        int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const char* who = "binary_search";
    if (int e = bin_check_search(who, queries, Q, dim, codes, G, out_val, out_idx)) return e;
    MI355_REQUIRE(k >= 1 && k <= LARGE_K && (G == 0 || k <= G), "%s: k=%d outside [1, %lld]", who, k,
                  (long long)(G > 0 && G < LARGE_K ? G : LARGE_K));
    RankFilter fall{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &fall)) return e;
    if (Q == 0 || G == 0) return OK;
    const BinWs w = bin_carve(workspace, Q, G, dim, k);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const bool fused = k <= SMALL_K;
    RoctxRange range(fused ? "binary/scan + per-chunk top-k" : "binary/scan + per-chunk top-8 + saturated chunks + top-k");
    const int ld = bin_ld(dim), ldq = bin_ldq(ld);
    if (int e = launch_encode(queries, Q, dim, 0, eps, center, w.qcodes, ldq, w.qnan, st)) return e;
    set_rank_path(MI355_RANK_PATH_BINARY | (fused ? MI355_RANK_PATH_FUSED : MI355_RANK_PATH_BITONIC));
    const i64 qb = bin_query_block(Q, G, k), nch = (G + BIN_CHUNK - 1) / BIN_CHUNK, cand_ld = bin_cand_ld(G, k);
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = Q - q0 < qb ? Q - q0 : qb;
        const RankFilter fb = filter ? filter_from(fall, q0) : RankFilter{};
        const RankFilter* f = filter ? &fb : nullptr;
        float* ov = out_val + q0 * k;
        i64* oi = (i64*)out_idx + q0 * k;
        BinScanArgs a{};
        a.codes = (const unsigned*)codes; a.G = G; a.ld = ld;
        a.qcodes = w.qcodes + q0 * ldq; a.qnan = w.qnan + q0; a.Q = (int)qn; a.ldq = ldq; a.dim = dim; a.nch = (int)nch;
        a.k = fused ? k : SMALL_K; a.idx_offset = idx_offset;
        a.cand_val = w.cand_val; a.cand_idx = w.cand_idx; a.cand_ld = cand_ld; a.flt = fb;
        if (int e = f ? dispatch_fused<true>(a, st) : dispatch_fused<false>(a, st)) return e;
        if (!fused) {
            BinRescanArgs r{};
            r.codes = a.codes; r.G = G; r.ld = ld; r.qcodes = a.qcodes; r.qnan = a.qnan; r.ldq = ldq; r.dim = dim;
            r.idx_offset = idx_offset; r.cand_ld = cand_ld; r.cand_val = w.cand_val; r.cand_idx = w.cand_idx; r.flt = fb;
            if (int e = bin_saturated_route<false>(r, qn, nch, k, f, ov, oi, w.satlist, w.satcount, w.topk, w.topk_bytes, st)) return e;
        }
        // the candidates carry their indices; with a filter the slots no eligible row filled end as (-inf, -1)
        if (int e = topk_select(w.cand_val, w.cand_idx, qn, cand_ld, cand_ld, k, 0, ov, oi, w.topk, w.topk_bytes, st, nullptr, f)) return e;
    }
    return OK;
}

size_t mi355_binary_asym_search_workspace_bytes(int64_t Q, int64_t G, int dim, int k) {
    if (Q < 1 || !bin_shape_ok(Q, G, dim) || k < 0 || k > LARGE_K) return 0;
    return bin_asym_carve(nullptr, Q, G, dim, k).total;
}

int mi355_binary_asym_query_codes(const float* queries, int64_t Q, int dim, float eps, const float* center, int8_t* codes, int32_t* l1,
                                  int32_t* nanflag, void* stream) {
    const char* who = "binary_asym_query_codes";
    MI355_REQUIRE(queries && codes && l1 && nanflag, "%s: null pointer", who);
    MI355_REQUIRE(Q >= 0 && dim >= 1, "%s: bad shape Q=%lld dim=%d", who, (long long)Q, dim);
    MI355_REQUIRE(dim <= BIN_MAX_DIM, "%s: dim=%d exceeds %d", who, dim, BIN_MAX_DIM);
    MI355_REQUIRE(Q <= INT_MAX, "%s: shape too large Q=%lld", who, (long long)Q);
    if (Q == 0) return OK;
    RoctxRange range("binary/asymmetric query codes");
    return launch_asym_queries(queries, Q, Q, dim, eps, center, nullptr, nullptr, (int*)l1, (int*)nanflag, (signed char*)codes,
                               (hipStream_t)stream);
}

int mi355_binary_asym_distances(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G,
                                int32_t* dist, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "binary_asym_distances";
    if (int e = bin_check_search(who, queries, Q, dim, codes, G, dist, dist)) return e;
    if (Q == 0 || G == 0) return OK;
    const BinAsymWs w = bin_asym_carve(workspace, Q, G, dim, 0);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("binary/asymmetric distances");
    if (int e = launch_asym_queries(queries, Q, (Q + 31) / 32 * 32, dim, eps, center, w.frag, w.upos, w.l1, w.qnan, nullptr, st)) return e;
    const int ld = bin_ld(dim);
    const i64 qb = bin_query_block(Q, G, 0), nch = (G + BIN_CHUNK - 1) / BIN_CHUNK;
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = Q - q0 < qb ? Q - q0 : qb;
        BinAsymScanArgs b{};
        b.s.codes = (const unsigned*)codes; b.s.G = G; b.s.ld = ld; b.s.Q = (int)qn; b.s.dim = dim; b.s.nch = (int)nch;
        b.s.out = (int*)dist + q0 * G; b.s.ld_out = G;
        b.aq = asym_queries(w, dim); b.aq0 = (int)q0; b.S = ld < BIN_SLICE ? ld : BIN_SLICE;
        if (int e = launch_asym_scan<BIN_DIST, 1, false>(b, st)) return e;
    }
    return OK;
}

int mi355_binary_asym_search(const float* queries, int64_t Q, int dim, float eps, const float* center, const void* codes, int64_t G, int k,
                             int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const char* who = "binary_asym_search";
    if (int e = bin_check_search(who, queries, Q, dim, codes, G, out_val, out_idx)) return e;
    MI355_REQUIRE(k >= 1 && k <= LARGE_K && (G == 0 || k <= G), "%s: k=%d outside [1, %lld]", who, k,
                  (long long)(G > 0 && G < LARGE_K ? G : LARGE_K));
    RankFilter fall{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &fall)) return e;
    if (Q == 0 || G == 0) return OK;
    const BinAsymWs w = bin_asym_carve(workspace, Q, G, dim, k);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const bool fused = k <= SMALL_K;
    RoctxRange range(fused ? "binary/asymmetric scan + per-chunk top-k"
                           : "binary/asymmetric scan + per-chunk top-8 + saturated chunks + top-k");
    if (int e = launch_asym_queries(queries, Q, (Q + 31) / 32 * 32, dim, eps, center, w.frag, w.upos, w.l1, w.qnan, nullptr, st)) return e;
    set_rank_path(MI355_RANK_PATH_BINARY_ASYM | (fused ? MI355_RANK_PATH_FUSED : MI355_RANK_PATH_BITONIC));
    const int ld = bin_ld(dim);
    const i64 qb = bin_query_block(Q, G, k), nch = (G + BIN_CHUNK - 1) / BIN_CHUNK, cand_ld = bin_cand_ld(G, k);
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = Q - q0 < qb ? Q - q0 : qb;
        const RankFilter fb = filter ? filter_from(fall, q0) : RankFilter{};
        const RankFilter* f = filter ? &fb : nullptr;
        float* ov = out_val + q0 * k;
        i64* oi = (i64*)out_idx + q0 * k;
        BinAsymScanArgs b{};
        b.s.codes = (const unsigned*)codes; b.s.G = G; b.s.ld = ld; b.s.Q = (int)qn; b.s.dim = dim; b.s.nch = (int)nch;
        b.s.k = fused ? k : SMALL_K; b.s.idx_offset = idx_offset;
        b.s.cand_val = w.cand_val; b.s.cand_idx = w.cand_idx; b.s.cand_ld = cand_ld; b.s.flt = fb;
        b.aq = asym_queries(w, dim); b.aq0 = (int)q0; b.S = ld < BIN_SLICE ? ld : BIN_SLICE;
        if (int e = f ? dispatch_asym_fused<true>(b, st) : dispatch_asym_fused<false>(b, st)) return e;
        if (!fused) {
            BinRescanArgs r{};
            r.codes = b.s.codes; r.G = G; r.ld = ld; r.dim = dim; r.aq = b.aq; r.aq0 = b.aq0;
            r.idx_offset = idx_offset; r.cand_ld = cand_ld; r.cand_val = w.cand_val; r.cand_idx = w.cand_idx; r.flt = fb;
            if (int e = bin_saturated_route<true>(r, qn, nch, k, f, ov, oi, w.satlist, w.satcount, w.topk, w.topk_bytes, st)) return e;
        }
        if (int e = topk_select(w.cand_val, w.cand_idx, qn, cand_ld, cand_ld, k, 0, ov, oi, w.topk, w.topk_bytes, st, nullptr, f)) return e;
    }
    return OK;
}

}  // extern "C"
