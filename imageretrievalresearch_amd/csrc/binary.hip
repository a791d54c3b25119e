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
// No atomics: every output slot has one writer.  gfx950 only.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

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

// Words [s0, s0 + S) of the chunk's 256 rows into rows_s [256][S + 1]; a row past G or a word past ld reads as 0
template <int S>
__device__ __forceinline__ void bin_stage(unsigned* rows_s, const BinScanArgs& a, i64 c0, int s0) {
    constexpr int PPR = S / 4;                                          // 16-byte pieces of a row slice
    for (int p = threadIdx.x; p < BIN_CHUNK * PPR; p += 256) {
        const int row = p / PPR, w0 = s0 + (p - row * PPR) * 4;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c0 + row < a.G && w0 < a.ld) v = *reinterpret_cast<const uint4*>(a.codes + (c0 + row) * a.ld + w0);
        unsigned* d = rows_s + row * (S + 1) + (w0 - s0);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
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
            // thread t: query t / 8 of the pass, keys part * 33 .. part * 33 + 31 of it (rows part * 32 .. + 31 of the chunk)
            const int qq = tid >> 3, part = tid & 7;
            unsigned kv[K];
#pragma unroll
            for (int i = 0; i < K; ++i) kv[i] = BIN_NO_KEY;
            auto insert = [&](unsigned key) {                           // keys are distinct; BIN_NO_KEY is below nothing
                bool g[K];
#pragma unroll
                for (int i = 0; i < K; ++i) g[i] = key < kv[i];
#pragma unroll
                for (int i = K - 1; i > 0; --i) kv[i] = g[i] ? (g[i - 1] ? kv[i - 1] : key) : kv[i];
                kv[0] = g[0] ? key : kv[0];
            };
            if (qq < nq) {                                              // (whole groups of 8 lanes: the shuffles below stay inside one)
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
            if (part == 0 && qq < nq) {
                const int q = qp + qq;
                const bool qbad = a.qnan[q] != 0;
                const size_t o = (size_t)q * a.cand_ld + (size_t)chunk * a.k;
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    if (i < a.k) {
                        const bool have = kv[i] != BIN_NO_KEY;
                        const float s = qbad ? __uint_as_float(0x7fc00000u) : bin_score((int)(kv[i] >> 8), a.dim);
                        a.cand_val[o + i] = have ? s : NEG_INF;
                        a.cand_idx[o + i] = have ? c0 + (i64)(kv[i] & 255u) + a.idx_offset : IDX_PAD;
                    }
                }
            }
            __syncthreads();                                            // the next pass writes the tile
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
};
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
            const unsigned* qw = a.qcodes + q * a.ldq;
            int h = 0;
            for (int w = 0; w < a.ld; ++w) h += __popc(g[w] ^ qw[w]);
            val = a.qnan[q] ? __uint_as_float(0x7fc00000u) : bin_score(h, a.dim);
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
            // the bound: the k-th best of the chunks' candidates, into the output for now (none if there are fewer than k)
            const i64 head = nch * SMALL_K;
            const bool bound = head >= k;
            if (bound)
                if (int e = topk_select(w.cand_val, w.cand_idx, qn, head, cand_ld, k, 0, ov, oi, w.topk, w.topk_bytes, st, nullptr, f))
                    return e;
            const int nslots = k / SMALL_K;
            hipLaunchKernelGGL(k_bin_saturated, dim3((unsigned)qn), dim3(256), 0, st, w.cand_val, w.cand_idx, cand_ld, (int)nch,
                               bound ? ov : nullptr, bound ? oi : nullptr, k, nslots, w.satlist, w.satcount);
            MI355_LAUNCH_CHECK();
            BinRescanArgs r{};
            r.codes = a.codes; r.G = G; r.ld = ld; r.qcodes = a.qcodes; r.qnan = a.qnan; r.ldq = ldq; r.dim = dim; r.nslots = nslots;
            r.satlist = w.satlist; r.satcount = w.satcount; r.idx_offset = idx_offset; r.cand_ld = cand_ld; r.tail = head;
            r.cand_val = w.cand_val; r.cand_idx = w.cand_idx; r.flt = fb; r.filt = f ? 1 : 0;
            hipLaunchKernelGGL(k_bin_rescan, dim3((unsigned)nslots, (unsigned)qn), dim3(256), 0, st, r);
            MI355_LAUNCH_CHECK();
        }
        // the candidates carry their indices; with a filter the slots no eligible row filled end as (-inf, -1)
        if (int e = topk_select(w.cand_val, w.cand_idx, qn, cand_ld, cand_ld, k, 0, ov, oi, w.topk, w.topk_bytes, st, nullptr, f)) return e;
    }
    return OK;
}

}  // extern "C"
