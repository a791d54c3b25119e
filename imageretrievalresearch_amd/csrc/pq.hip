// Product-quantised (PQ) resident gallery: a row is M bytes, byte m the nearest of the 256 centroids of sub-quantiser m over the
// row's sub-vector m.  The arithmetic of every kernel here is specified bit for bit in include/mi355_retrieval.h:
//   k_pq_encode ... codebook m in LDS, one thread per row: the nearest centroid in plain VALU fp32 (sub, mul, add each rounded)
//   k_pq_update ... one workgroup per cell (m, c): the float64 sum of its members' sub-vectors in ascending row order
//   k_pq_table .... T[q][m][c] = qn[q] sub-vector m . centroid (m, c), multiply and add rounded separately
//   k_pq_scan ..... one workgroup per (query, chunk of PQ_CHUNK rows), the query's table in LDS (M KB): M lookups per row into
//                   four accumulators, then the small-k selection of rank_topk_small.inc over scores that never reach memory
//   k_pq_scores ... the same lookups, written out as a score slab (k > 8, mi355_pq_scores)
//   k_rescore ..... one wave per (query, candidate): the row dot of the IVF scan (row_dot.h) against fp32 / fp16 rows
// The table in LDS, the lookups of one row and the shape rules live in pq_scan.h: the IVF-PQ scan (ivfpq.hip) shares them.
// No atomics: every output slot has one writer.  gfx950 only.
#include "pq_scan.h"
#include "row_dot.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

constexpr int PQ_CHUNK = 2048;              // rows of one scan workgroup; the table load (M KB) is 1/8 of its lookups
constexpr int PQ_TABLE_Q = 8;               // queries of one table workgroup: codebook m is staged in LDS once for them
constexpr i64 PQ_ENC_BLOCK = 16384;         // rows normalised at a time by mi355_pq_encode
constexpr int PQ_UPD_ROWS = 4096;           // rows one pass of k_pq_update looks at: 16 per thread
constexpr int RESCORE_CHUNK = 64;           // candidates of one rescore workgroup: 16 per wave
constexpr size_t RESCORE_LDS = 64 * 1024;   // the query
constexpr i64 RESCORE_QBLOCK = 32768;       // queries of one launch (grid.y)

// The value as it is, but in a register of its own: the compiler cannot fold the multiply that made it into a following add
// (-ffp-contract=fast would turn mul + add into one fma, i.e. one rounding where the contract names two).  Emits nothing.
__device__ __forceinline__ float pinned(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// ---- encode: grid (cdiv(R, 256), M); n [R][dim] normalised rows; codes [R][M].  DMAX >= dsub: the sub-vector's registers
template <int DMAX>
__global__ __launch_bounds__(256) void k_pq_encode(const float* __restrict__ n, const float* __restrict__ cb,
                                                   unsigned char* __restrict__ codes, i64 R, int dim, int M) {
    extern __shared__ __attribute__((aligned(16))) float cbs[];    // [256][dsub]: codebook m
    const int m = blockIdx.y, dsub = dim / M;
    const float* src = cb + (size_t)m * PQ_CENTROIDS * dsub;
    for (int i = threadIdx.x; i < PQ_CENTROIDS * dsub; i += 256) cbs[i] = src[i];
    __syncthreads();
    const i64 g = (i64)blockIdx.x * 256 + threadIdx.x;
    if (g >= R) return;
    const float* row = n + g * dim + (i64)m * dsub;
    float x[DMAX];
#pragma unroll
    for (int i = 0; i < DMAX; ++i) x[i] = i < dsub ? row[i] : 0.f;
    float best = INFINITY;                                          // a NaN distance is never below it
    int code = 0;
    for (int c = 0; c < PQ_CENTROIDS; ++c) {
        const float* b = cbs + c * dsub;                            // the same address in every lane: a broadcast read
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < DMAX; ++i) {
            if (i < dsub) {                                         // (uniform: a scalar branch)
                const float t = __fsub_rn(x[i], b[i]);
                d = __fadd_rn(d, pinned(__fmul_rn(t, t)));
            }
        }
        if (d < best) { best = d; code = c; }                       // strict: the lowest c among equals
    }
    codes[g * M + m] = (unsigned char)code;
}

// ---- centroid update: grid (256, M), one workgroup per cell (c, m).  PQ_UPD_ROWS rows per pass: thread t looks at the 16 rows
// t * 16 .. t * 16 + 15 of the pass, the members go to LDS in ascending row order (a prefix over the threads), and thread i <
// dsub adds element i of each member's sub-vector to its float64 sum, one member after the other.
__global__ __launch_bounds__(256) void k_pq_update(const float* __restrict__ n, const unsigned char* __restrict__ codes,
                                                   const float* cb, float* cb_out, i64* __restrict__ counts, i64 R, int dim,
                                                   int M) {
    __shared__ int members[PQ_UPD_ROWS];
    __shared__ int wave_cnt[4];
    const int c = blockIdx.x, m = blockIdx.y, dsub = dim / M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double sum = 0.0;
    i64 count = 0;
    for (i64 r0 = 0; r0 < R; r0 += PQ_UPD_ROWS) {
        unsigned mask = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const i64 r = r0 + tid * 16 + j;
            if (r < R && codes[r * M + m] == c) mask |= 1u << j;
        }
        const int mine = __popc(mask);
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wave_cnt[wave] = incl;
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) base += wave_cnt[w];
            total += wave_cnt[w];
        }
        int pos = base + incl - mine;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((mask >> j) & 1u) members[pos++] = tid * 16 + j;    // pos < total <= PQ_UPD_ROWS
        __syncthreads();
        if (tid < dsub) {
            const float* col = n + r0 * dim + (i64)m * dsub + tid;
            for (int t = 0; t < total; ++t) sum += (double)col[(i64)members[t] * dim];
        }
        count += total;
        __syncthreads();                                            // members and wave_cnt are rewritten by the next pass
    }
    if (tid < dsub) {
        const size_t o = ((size_t)m * PQ_CENTROIDS + c) * dsub + tid;
        cb_out[o] = count > 0 ? (float)(sum / (double)count) : cb[o];
    }
    if (tid == 0) counts[m * PQ_CENTROIDS + c] = count;
}

// ---- table: grid (M, cdiv(queries, PQ_TABLE_Q)), thread c.  Codebook m goes to LDS with coalesced loads, rows dsub | 1 floats
// apart (an odd stride: the 32 lanes of a read hit 32 banks), and serves PQ_TABLE_Q queries.
__global__ __launch_bounds__(256) void k_pq_table(const float* __restrict__ qn, const float* __restrict__ cb, float* __restrict__ T,
                                                  int dim, int M, i64 Q) {
    extern __shared__ __attribute__((aligned(16))) float cbs[];    // [256][dsub | 1]
    const int m = blockIdx.x, c = threadIdx.x, dsub = dim / M, ldc = dsub | 1;
    const float* src = cb + (size_t)m * PQ_CENTROIDS * dsub;
    for (int i = threadIdx.x; i < PQ_CENTROIDS * dsub; i += 256) {
        const int cc = i / dsub;
        cbs[cc * ldc + (i - cc * dsub)] = src[i];
    }
    __syncthreads();
    const float* b = cbs + c * ldc;
    const i64 q0 = (i64)blockIdx.y * PQ_TABLE_Q, q1 = q0 + PQ_TABLE_Q < Q ? q0 + PQ_TABLE_Q : Q;
    for (i64 q = q0; q < q1; ++q) {
        const float* x = qn + q * dim + (i64)m * dsub;              // the same address in every lane
        float acc = 0.f;
        for (int i = 0; i < dsub; ++i) acc = __fadd_rn(acc, pinned(__fmul_rn(x[i], b[i])));
        T[(q * M + m) * PQ_CENTROIDS + c] = acc;
    }
}

// ---- scan with the selection inside (k <= K <= 8): grid (cdiv(G, PQ_CHUNK), queries).  The body is the small-k selection of
// the score slabs; its candidate value is the row's lookups.  ov / oi [queries][chunks][k].
template <int K, bool FILT, bool VEC, int NT>
__global__ __launch_bounds__(NT) void k_pq_scan(const float* __restrict__ T, const unsigned char* __restrict__ codes, i64 G, int M,
                                                 int k, i64 idx_offset, float* __restrict__ ov, i64* __restrict__ oi,
                                                 RankFilter flt) {
    extern __shared__ __attribute__((aligned(16))) float tab[];    // [M][256]
    pq_load_table<NT>(tab, T, M);
    const float* const vals = nullptr;
    const i64* const idxs = nullptr;
    const int* const idxs32 = nullptr;
    const i64 rowlen = G, in_stride = 0, chunk_len = PQ_CHUNK;
#define TOPK_SMALL_VALUE(j) ((void)v, pq_score<VEC>(tab, codes, (j), M))
#define TOPK_SMALL_THREADS NT
#include "rank_topk_small.inc"
#undef TOPK_SMALL_THREADS
#undef TOPK_SMALL_VALUE
}

// ---- the score slab S [queries][ldS]: the same grid, every row of the chunk written by one thread
template <bool VEC, int NT>
__global__ __launch_bounds__(NT) void k_pq_scores(const float* __restrict__ T, const unsigned char* __restrict__ codes, i64 G, int M,
                                                   float* __restrict__ S, i64 ldS) {
    extern __shared__ __attribute__((aligned(16))) float tab[];    // [M][256]
    pq_load_table<NT>(tab, T, M);
    const i64 c0 = (i64)blockIdx.x * PQ_CHUNK, c1 = c0 + PQ_CHUNK < G ? c0 + PQ_CHUNK : G;
    float* out = S + (i64)blockIdx.y * ldS;
    for (i64 j = c0 + threadIdx.x; j < c1; j += NT) out[j] = pq_score<VEC>(tab, codes, j, M);
}

// ---- rescoring: grid (cdiv(R, RESCORE_CHUNK), queries); the query in LDS, wave w takes candidates w, w + 4, ... of the chunk
struct RescoreArgs {
    const float* qn;        // [Q][dim] normalised queries
    const void* rows;
    i64 ld, G;
    int dim, ldq;
    const i64* cand;        // [Q][R]
    i64 R, idx_offset;
    float* out;             // [Q][R]
};
template <bool F16, bool VEC>
__global__ __launch_bounds__(256) void k_rescore(RescoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) float qs[];     // [ldq]
    const i64 q = blockIdx.y;
    for (int i = threadIdx.x; i < a.ldq; i += 256) qs[i] = i < a.dim ? a.qn[q * a.dim + i] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 r0 = (i64)blockIdx.x * RESCORE_CHUNK, r1 = r0 + RESCORE_CHUNK < a.R ? r0 + RESCORE_CHUNK : a.R;
    for (i64 r = r0 + wave; r < r1; r += 4) {
        const i64 ci = a.cand[q * a.R + r];
        const i64 g = (i64)((unsigned long long)ci - (unsigned long long)a.idx_offset);
        const bool ok = ci >= 0 && ci < NO_CAND_IDX && g >= 0 && g < a.G;      // the same for the whole wave
        float acc[1] = {0.f};
        if (ok) row_dot<1, F16, VEC>(a, g, qs, lane, acc);
        const float t = wave_sum(acc[0]);
        if (lane == 0) a.out[q * a.R + r] = ok ? t : NEG_INF;
    }
}

// ---- host side
// Scratch of a search over Q queries (k = 0: mi355_pq_scores, no selection): the normalised queries, the tables of one query
// block, then the block's candidate lists (k <= 8) or its score slab (k > 8) and the selection's own scratch
struct PqWs {
    float* qn; float* T; float* S; float* cand_val; i64* cand_idx; void* topk; size_t topk_bytes; size_t total;
};
static i64 pq_query_block(i64 Q, i64 G, int k) {
    i64 qb = PQ_QBLOCK;
    if (k > SMALL_K) {
        const i64 fit = PQ_SLAB_FLOATS / (G > 0 ? G : 1);
        if (fit < qb) qb = fit < 1 ? 1 : fit;
    }
    return qb < Q ? qb : Q;
}
static PqWs pq_carve(void* ws, i64 Q, i64 G, int dim, int M, int k) {
    PqWs r{};
    WsCarver c(ws);
    const i64 qb = pq_query_block(Q, G, k);
    r.qn = (float*)c.take((size_t)Q * dim * sizeof(float));
    r.T = (float*)c.take((size_t)qb * M * PQ_CENTROIDS * sizeof(float));
    if (k >= 1 && k <= SMALL_K) {
        const size_t n = (size_t)qb * cdiv(G, PQ_CHUNK) * k;
        r.cand_val = (float*)c.take(n * sizeof(float));
        r.cand_idx = (i64*)c.take(n * sizeof(i64));
        r.topk_bytes = topk_ws_bytes(qb, (i64)cdiv(G, PQ_CHUNK) * k, k);
        r.topk = c.take(r.topk_bytes);
    } else if (k > SMALL_K) {
        r.S = (float*)c.take((size_t)qb * G * sizeof(float));
        r.topk_bytes = topk_ws_bytes(qb, G, k);
        r.topk = c.take(r.topk_bytes);
    }
    r.total = c.total();
    return r;
}

// The scan kernels ask for up to 128 KB of dynamic LDS: raise each one's limit once per device
template <class Kern>
static int pq_allow_lds(Kern kern, bool* done) {
    if (first_time_on_this_device(done))
        MI355_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, PQ_MAX_M * 1024));
    return OK;
}
template <int K, bool FILT, bool VEC, int NT>
static int launch_scan_nt(dim3 grid, const float* T, const unsigned char* codes, i64 G, int M, int k, i64 idx_offset, float* ov, i64* oi,
                          const RankFilter& f, hipStream_t st) {
    static bool done[MI355_MAX_DEVICES] = {false};
    if (int e = pq_allow_lds(k_pq_scan<K, FILT, VEC, NT>, done)) return e;
    hipLaunchKernelGGL((k_pq_scan<K, FILT, VEC, NT>), grid, dim3(NT), (size_t)M * 1024, st, T, codes, G, M, k, idx_offset, ov, oi, f);
    MI355_LAUNCH_CHECK();
    return OK;
}
template <int K, bool FILT, bool VEC>
static int launch_scan(dim3 grid, const float* T, const unsigned char* codes, i64 G, int M, int k, i64 idx_offset, float* ov, i64* oi,
                       const RankFilter& f, hipStream_t st) {
    const int nt = pq_threads(M);
    if (nt == 256) return launch_scan_nt<K, FILT, VEC, 256>(grid, T, codes, G, M, k, idx_offset, ov, oi, f, st);
    if (nt == 512) return launch_scan_nt<K, FILT, VEC, 512>(grid, T, codes, G, M, k, idx_offset, ov, oi, f, st);
    return launch_scan_nt<K, FILT, VEC, 1024>(grid, T, codes, G, M, k, idx_offset, ov, oi, f, st);
}
template <bool FILT, bool VEC>
static int dispatch_scan(dim3 grid, const float* T, const unsigned char* codes, i64 G, int M, int k, i64 idx_offset, float* ov, i64* oi,
                         const RankFilter& f, hipStream_t st) {
    if (k <= 1) return launch_scan<1, FILT, VEC>(grid, T, codes, G, M, k, idx_offset, ov, oi, f, st);
    if (k <= 2) return launch_scan<2, FILT, VEC>(grid, T, codes, G, M, k, idx_offset, ov, oi, f, st);
    if (k <= 4) return launch_scan<4, FILT, VEC>(grid, T, codes, G, M, k, idx_offset, ov, oi, f, st);
    return launch_scan<8, FILT, VEC>(grid, T, codes, G, M, k, idx_offset, ov, oi, f, st);
}
template <bool VEC, int NT>
static int launch_scores_nt(dim3 grid, const float* T, const unsigned char* codes, i64 G, int M, float* S, i64 ldS, hipStream_t st) {
    static bool done[MI355_MAX_DEVICES] = {false};
    if (int e = pq_allow_lds(k_pq_scores<VEC, NT>, done)) return e;
    hipLaunchKernelGGL((k_pq_scores<VEC, NT>), grid, dim3(NT), (size_t)M * 1024, st, T, codes, G, M, S, ldS);
    MI355_LAUNCH_CHECK();
    return OK;
}
template <bool VEC>
static int launch_scores(dim3 grid, const float* T, const unsigned char* codes, i64 G, int M, float* S, i64 ldS, hipStream_t st) {
    const int nt = pq_threads(M);
    if (nt == 256) return launch_scores_nt<VEC, 256>(grid, T, codes, G, M, S, ldS, st);
    if (nt == 512) return launch_scores_nt<VEC, 512>(grid, T, codes, G, M, S, ldS, st);
    return launch_scores_nt<VEC, 1024>(grid, T, codes, G, M, S, ldS, st);
}
int launch_table(const float* qn_rows, i64 qn, int dim, const float* cb, int M, float* T, hipStream_t st) {
    static bool done[MI355_MAX_DEVICES] = {false};
    if (int e = pq_allow_lds(k_pq_table, done)) return e;         // 256 * 65 floats at dsub = 64: just above 64 KB
    const size_t lds = (size_t)PQ_CENTROIDS * ((dim / M) | 1) * sizeof(float);
    hipLaunchKernelGGL(k_pq_table, dim3((unsigned)M, (unsigned)cdiv(qn, PQ_TABLE_Q)), dim3(256), lds, st, qn_rows, cb, T, dim, M, qn);
    MI355_LAUNCH_CHECK();
    return OK;
}

// The tables of queries [q0, q0 + qn) into T, then their scores against the G code rows into S [qn][ldS]
static int pq_scores_block(const float* qn_rows, i64 qn, int dim, const float* cb, int M, const unsigned char* codes, i64 G, float* T,
                           float* S, i64 ldS, hipStream_t st) {
    if (int e = launch_table(qn_rows, qn, dim, cb, M, T, st)) return e;
    const dim3 grid((unsigned)cdiv(G, PQ_CHUNK), (unsigned)qn);
    return M % 16 == 0 ? launch_scores<true>(grid, T, codes, G, M, S, ldS, st) : launch_scores<false>(grid, T, codes, G, M, S, ldS, st);
}

// What mi355_pq_scores and mi355_pq_search check of their common arguments
static int pq_check_search(const char* who, const void* queries, i64 Q, int dim, const void* codebooks, int M, const void* codes, i64 G,
                           const void* out0, const void* out1) {
    MI355_REQUIRE(queries && codebooks && codes && out0 && out1, "%s: null pointer", who);
    MI355_REQUIRE(Q >= 0 && G >= 0 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    if (int e = pq_check_shape(who, dim, M)) return e;
    MI355_REQUIRE(((uintptr_t)codes & 15) == 0, "%s: gallery buffer must be 16-byte aligned", who);
    MI355_REQUIRE(Q <= INT_MAX && G <= ((i64)1 << 40), "%s: shape too large Q=%lld G=%lld", who, (long long)Q, (long long)G);
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_pq_encode_workspace_bytes(int64_t R, int dim, int rows_are_normalized) {
    if (R < 1 || dim < 1 || rows_are_normalized) return 0;
    return (size_t)(R < PQ_ENC_BLOCK ? R : PQ_ENC_BLOCK) * dim * sizeof(float) + 256;
}

int mi355_pq_encode(const float* rows, int64_t R, int dim, int M, int rows_are_normalized, float eps, const float* codebooks,
                    void* codes, size_t codes_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pq_encode";
    MI355_REQUIRE(rows && codebooks && codes, "%s: null pointer", who);
    MI355_REQUIRE(R >= 0 && dim >= 1, "%s: bad shape R=%lld dim=%d", who, (long long)R, dim);
    if (int e = pq_check_shape(who, dim, M)) return e;
    MI355_REQUIRE(R <= ((int64_t)1 << 40), "%s: shape too large R=%lld", who, (long long)R);
    MI355_REQUIRE(codes_bytes >= (size_t)R * M, "%s: output buffer %zu < %zu bytes", who, codes_bytes, (size_t)R * M);
    const size_t need = mi355_pq_encode_workspace_bytes(R, dim, rows_are_normalized);
    MI355_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    if (R == 0) return OK;
    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("pq/encode");
    float* nbuf = rows_are_normalized ? nullptr : (float*)align256(workspace);
    const size_t lds = (size_t)PQ_CENTROIDS * (dim / M) * sizeof(float);
    for (int64_t r0 = 0; r0 < R; r0 += PQ_ENC_BLOCK) {
        const int64_t rn = R - r0 < PQ_ENC_BLOCK ? R - r0 : PQ_ENC_BLOCK;
        const float* n = rows + r0 * dim;
        if (nbuf) {
            if (int e = mi355_l2_normalize_rows(n, nbuf, rn, dim, eps, stream)) return e;
            n = nbuf;
        }
        const dim3 grid((unsigned)cdiv(rn, 256), (unsigned)M);
        unsigned char* out = (unsigned char*)codes + r0 * M;
        if (dim / M <= 8) hipLaunchKernelGGL(k_pq_encode<8>, grid, dim3(256), lds, st, n, codebooks, out, (i64)rn, dim, M);
        else if (dim / M <= 16) hipLaunchKernelGGL(k_pq_encode<16>, grid, dim3(256), lds, st, n, codebooks, out, (i64)rn, dim, M);
        else if (dim / M <= 32) hipLaunchKernelGGL(k_pq_encode<32>, grid, dim3(256), lds, st, n, codebooks, out, (i64)rn, dim, M);
        else hipLaunchKernelGGL(k_pq_encode<PQ_MAX_DSUB>, grid, dim3(256), lds, st, n, codebooks, out, (i64)rn, dim, M);
        MI355_LAUNCH_CHECK();
    }
    return OK;
}

size_t mi355_pq_update_workspace_bytes(int64_t R, int dim, int rows_are_normalized) {
    if (R < 1 || dim < 1 || rows_are_normalized) return 0;
    return (size_t)R * dim * sizeof(float) + 256;
}

int mi355_pq_update(const float* rows, int64_t R, int dim, int M, int rows_are_normalized, float eps, const void* codes,
                    const float* codebooks, float* codebooks_out, int64_t* counts, void* workspace, size_t workspace_bytes,
                    void* stream) {
    const char* who = "pq_update";
    MI355_REQUIRE(rows && codes && codebooks && codebooks_out && counts, "%s: null pointer", who);
    MI355_REQUIRE(R >= 0 && dim >= 1, "%s: bad shape R=%lld dim=%d", who, (long long)R, dim);
    if (int e = pq_check_shape(who, dim, M)) return e;
    MI355_REQUIRE(R <= ((int64_t)1 << 40), "%s: shape too large R=%lld", who, (long long)R);
    MI355_REQUIRE(((uintptr_t)codes & 15) == 0, "%s: gallery buffer must be 16-byte aligned", who);
    const size_t need = mi355_pq_update_workspace_bytes(R, dim, rows_are_normalized);
    MI355_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    if (R == 0) return OK;
    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("pq/update");
    const float* n = rows;
    if (!rows_are_normalized) {
        float* nbuf = (float*)align256(workspace);
        if (int e = mi355_l2_normalize_rows(rows, nbuf, R, dim, eps, stream)) return e;
        n = nbuf;
    }
    hipLaunchKernelGGL(k_pq_update, dim3(PQ_CENTROIDS, (unsigned)M), dim3(256), 0, st, n, (const unsigned char*)codes, codebooks,
                       codebooks_out, (i64*)counts, (i64)R, dim, M);
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t mi355_pq_search_workspace_bytes(int64_t Q, int64_t G, int dim, int M, int k) {
    if (Q < 1 || G < 0 || !pq_shape_ok(dim, M) || k < 0 || k > LARGE_K || Q > INT_MAX || G > ((int64_t)1 << 40)) return 0;
    return pq_carve(nullptr, Q, G, dim, M, k).total;
}

int mi355_pq_scores(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M, const void* codes, int64_t G,
                    float* scores, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pq_scores";
    if (int e = pq_check_search(who, queries, Q, dim, codebooks, M, codes, G, scores, scores)) return e;
    if (Q == 0 || G == 0) return OK;
    const PqWs w = pq_carve(workspace, Q, G, dim, M, 0);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("pq/scores");
    if (int e = mi355_l2_normalize_rows(queries, w.qn, Q, dim, eps, stream)) return e;
    const i64 qb = pq_query_block(Q, G, 0);
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = Q - q0 < qb ? Q - q0 : qb;
        if (int e = pq_scores_block(w.qn + q0 * dim, qn, dim, codebooks, M, (const unsigned char*)codes, G, w.T, scores + q0 * G, G, st))
            return e;
    }
    return OK;
}

int mi355_pq_search(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M, const void* codes, int64_t G,
                    int k, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, void* workspace,
                    size_t workspace_bytes, void* stream) {
    const char* who = "pq_search";
    if (int e = pq_check_search(who, queries, Q, dim, codebooks, M, codes, G, out_val, out_idx)) return e;
    MI355_REQUIRE(k >= 1 && k <= LARGE_K && (G == 0 || k <= G), "%s: k=%d outside [1, %lld]", who, k,
                  (long long)(G > 0 && G < LARGE_K ? G : LARGE_K));
    RankFilter fall{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &fall)) return e;
    if (Q == 0 || G == 0) return OK;
    const PqWs w = pq_carve(workspace, Q, G, dim, M, k);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* cd = (const unsigned char*)codes;
    const bool fused = k <= SMALL_K, vec = M % 16 == 0;
    RoctxRange range(fused ? "pq/scan + per-chunk top-k" : "pq/scan (score slab) + top-k");
    if (int e = mi355_l2_normalize_rows(queries, w.qn, Q, dim, eps, stream)) return e;
    set_rank_path(MI355_RANK_PATH_PQ | (fused ? MI355_RANK_PATH_FUSED : MI355_RANK_PATH_BITONIC));
    const i64 qb = pq_query_block(Q, G, k), nch = cdiv(G, PQ_CHUNK);
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = Q - q0 < qb ? Q - q0 : qb;
        const RankFilter fb = filter ? filter_from(fall, q0) : RankFilter{};
        const RankFilter* f = filter ? &fb : nullptr;
        float* ov = out_val + q0 * k;
        i64* oi = (i64*)out_idx + q0 * k;
        if (!fused) {
            if (int e = pq_scores_block(w.qn + q0 * dim, qn, dim, codebooks, M, cd, G, w.T, w.S, G, st)) return e;
            if (int e = topk_select(w.S, nullptr, qn, G, G, k, idx_offset, ov, oi, w.topk, w.topk_bytes, st, nullptr, f)) return e;
            continue;
        }
        if (int e = launch_table(w.qn + q0 * dim, qn, dim, codebooks, M, w.T, st)) return e;
        const dim3 grid((unsigned)nch, (unsigned)qn);
        int e;
        if (f) e = vec ? dispatch_scan<true, true>(grid, w.T, cd, G, M, k, idx_offset, w.cand_val, w.cand_idx, fb, st)
                       : dispatch_scan<true, false>(grid, w.T, cd, G, M, k, idx_offset, w.cand_val, w.cand_idx, fb, st);
        else e = vec ? dispatch_scan<false, true>(grid, w.T, cd, G, M, k, idx_offset, w.cand_val, w.cand_idx, fb, st)
                     : dispatch_scan<false, false>(grid, w.T, cd, G, M, k, idx_offset, w.cand_val, w.cand_idx, fb, st);
        if (e) return e;
        // the chunks' candidates carry their indices; with a filter the slots no eligible row filled end as (-inf, -1)
        if (int e2 = topk_select(w.cand_val, w.cand_idx, qn, nch * k, nch * k, k, 0, ov, oi, w.topk, w.topk_bytes, st, nullptr, f))
            return e2;
    }
    return OK;
}

size_t mi355_rescore_candidates_workspace_bytes(int64_t Q, int dim) {
    if (Q < 1 || dim < 1) return 0;
    return (size_t)Q * dim * sizeof(float) + 256;
}

int mi355_rescore_candidates(const float* queries, int64_t Q, int dim, float eps, const void* rows, int rows_dtype, int64_t ld,
                             int64_t G, const int64_t* cand_idx, int64_t R, int64_t idx_offset, float* out_val, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const char* who = "rescore_candidates";
    MI355_REQUIRE(queries && rows && cand_idx && out_val, "%s: null pointer", who);
    MI355_REQUIRE(rows_dtype == MI355_DTYPE_F32 || rows_dtype == MI355_DTYPE_F16, "%s: unknown rows dtype %d", who, rows_dtype);
    const bool f16rows = rows_dtype == MI355_DTYPE_F16;
    MI355_REQUIRE(Q >= 0 && G >= 0 && R >= 0 && dim >= 1, "%s: bad shape Q=%lld G=%lld R=%lld dim=%d", who, (long long)Q, (long long)G,
                  (long long)R, dim);
    MI355_REQUIRE(ld >= dim, "%s: ld=%lld < dim=%d", who, (long long)ld, dim);
    MI355_REQUIRE(!f16rows || (((uintptr_t)rows & 15) == 0 && ld % 8 == 0),
                  "%s: fp16 rows must be 16-byte aligned with ld=%lld a multiple of 8", who, (long long)ld);
    const int ldq = row_dot_ldq(dim, f16rows);
    MI355_REQUIRE((size_t)ldq * sizeof(float) <= RESCORE_LDS, "%s: dim=%d too large: one query of %d floats does not fit in %zu bytes "
                  "of LDS", who, dim, ldq, RESCORE_LDS);
    MI355_REQUIRE(R <= ((int64_t)1 << 31) && Q <= ((int64_t)1 << 40) / (R > 0 ? R : 1), "%s: shape too large Q=%lld R=%lld", who,
                  (long long)Q, (long long)R);
    const size_t need = mi355_rescore_candidates_workspace_bytes(Q, dim);
    MI355_REQUIRE(Q == 0 || (workspace && workspace_bytes >= need), "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    if (Q == 0 || R == 0) return OK;
    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("pq/rescore candidates");
    float* qn = (float*)align256(workspace);
    if (int e = mi355_l2_normalize_rows(queries, qn, Q, dim, eps, stream)) return e;
    const bool vec = ld % 4 == 0 && dim % 4 == 0 && ((uintptr_t)rows & 15) == 0;
    for (int64_t q0 = 0; q0 < Q; q0 += RESCORE_QBLOCK) {
        const int64_t qc = Q - q0 < RESCORE_QBLOCK ? Q - q0 : RESCORE_QBLOCK;
        RescoreArgs a{qn + q0 * dim, rows, ld, G, dim, ldq, (const i64*)cand_idx + q0 * R, R, idx_offset, out_val + q0 * R};
        const dim3 grid((unsigned)cdiv(R, RESCORE_CHUNK), (unsigned)qc);
        const size_t lds = (size_t)ldq * sizeof(float);
        if (f16rows) hipLaunchKernelGGL((k_rescore<true, true>), grid, dim3(256), lds, st, a);
        else if (vec) hipLaunchKernelGGL((k_rescore<false, true>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_rescore<false, false>), grid, dim3(256), lds, st, a);
        MI355_LAUNCH_CHECK();
    }
    return OK;
}

}  // extern "C"
