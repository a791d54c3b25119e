// Result diversification: maximal marginal relevance (Carbonell and Goldstein, SIGIR 1998) and greedy near-duplicate suppression
// over a query's shortlist.  include/mi355_retrieval.h states both stages.
//   mi355_shortlist_gram ... S[q] = the L x L Gram matrix of the gallery rows in query q's shortlist.  One workgroup of four
//                            waves per (query, pair of 64-slot tiles at or above the diagonal); wave (wi, wj) owns the 32 x 32
//                            quadrant of slots (64 ti + 32 wi ..) x (64 tj + 32 wj ..) as 2 x 2 tiles of v_mfma_f32_16x16x32_f16.
//                            The operands go from global memory straight into the MFMA registers, as regional.hip's candidate
//                            rows do: lane (c = lane & 15, g = lane >> 4) of k-step s holds elements 32 s + 8 g .. + 7 of the
//                            row in slot c of its 16-slot tile - 16 bytes of an fp16 row, or 32 bytes of an fp32 row rounded to
//                            fp16 (round-to-nearest-even) in registers.  The rows are gathered by index, so there is no
//                            contiguous panel to stage: a shortlist's rows are read 2 L / 64 times each, from the L2 after the
//                            first (L rows of 1536 fp16 are 3 MiB at L = 1024).  Measured: level with
//                            gather + torch.bmm at L = 100, behind it from L = 200 on - the loads bound it, and a larger tile
//                            staged through LDS is the known next step.
//                            The k-steps run in ascending column order whatever the tile or the slot, and every product of two
//                            fp16 values is exact in fp32: an entry's bits depend on its unordered pair of rows alone.  Below
//                            the diagonal nothing is computed: every entry at or above it is stored together with its mirror.
//   mi355_mmr_select ....... one workgroup per query (one wave where L <= 64), one shortlist slot per thread: the slot's
//                            relevance and its running maximum similarity to the picks stay in registers.  Every pick is an
//                            argmax over (value, position) keys by xor shuffles in the wave and one LDS round over the waves;
//                            the picked slot's Gram row is then read from global memory, where the first kernel left it.
// The selection arithmetic is compiled without contraction (the file's other code has none to contract).  No atomics, no host
// sync, ordinary vector stores.  gfx950 only.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef long long i64;
typedef _Float16 dv_f16x8 __attribute__((ext_vector_type(8)));
typedef float dv_f32x4 __attribute__((ext_vector_type(4)));

constexpr int DV_MAX_L = MI355_DIVERSIFY_MAX_SHORTLIST, DV_MAX_DIM = 65536;
constexpr int DV_TILE = 64, DV_THREADS = 256;      // a workgroup's tile of slots, four waves of 32 x 32 each

struct DvGramArgs {
    const void* rows;     // [G][ld] fp32 or fp16
    i64 ld, G;
    int dim;
    const i64* idx;       // [Q][L] local rows
    int L;
    float* out;           // [Q][L][L]
};

// Elements k .. k + 7 of the row that starts `off` elements into `rows`, as fp16, where all eight lie before dim.
template <bool F16, bool VEC>
__device__ __forceinline__ dv_f16x8 dv_load_full(const void* rows, i64 off, int k) {
    if constexpr (F16) {
        return *reinterpret_cast<const dv_f16x8*>(reinterpret_cast<const _Float16*>(rows) + off + k);
    } else {
        const float* p = reinterpret_cast<const float*>(rows) + off + k;
        float x[8];
        if constexpr (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = p[e];
        }
        dv_f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (_Float16)x[e];
        return v;
    }
}

// The same in the last, partial k-step: elements at or past dim are zero, and nothing past the row's stride is read (an fp16
// row's stride is a multiple of 8 and k < dim <= ld, so its 16 bytes at k lie inside the row).
template <bool F16>
__device__ __forceinline__ dv_f16x8 dv_load_tail(const void* rows, i64 off, int k, int dim) {
    dv_f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k >= dim) return v;
    if constexpr (F16) {
        v = *reinterpret_cast<const dv_f16x8*>(reinterpret_cast<const _Float16*>(rows) + off + k);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (k + e >= dim) v[e] = (_Float16)0;
    } else {
        const float* p = reinterpret_cast<const float*>(rows) + off + k;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (k + e < dim) v[e] = (_Float16)p[e];
    }
    return v;
}

template <bool F16, bool VEC>
__global__ __launch_bounds__(DV_THREADS) void k_shortlist_gram(DvGramArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, grp = lane >> 4, wi = wave >> 1, wj = wave & 1;
    const i64 q = blockIdx.x;
    const int nt = (a.L + DV_TILE - 1) / DV_TILE;
    int ti = 0, left = (int)blockIdx.y;               // pair number -> (ti, tj), ti <= tj: row ti of the triangle holds nt - ti pairs
    while (left >= nt - ti) { left -= nt - ti; ++ti; }
    const int tj = ti + left;
    if (ti == tj && wi > wj) return;                  // the mirror of quadrant (wj, wi), which stores both
    const int ibase = ti * DV_TILE + wi * 32, jbase = tj * DV_TILE + wj * 32;
    if (ibase >= a.L || jbase >= a.L) return;         // ibase <= jbase: a quadrant with no slot at all

    // this lane's rows: slot ibase + 16 t + c of the A side, jbase + 16 t + c of the B side; a pad reads row 0 and is zeroed below
    i64 offa[2], offb[2];
    bool oka[2], okb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int si = ibase + t * 16 + c, sj = jbase + t * 16 + c;
        const i64 ri = si < a.L ? a.idx[q * a.L + si] : -1, rj = sj < a.L ? a.idx[q * a.L + sj] : -1;
        oka[t] = ri >= 0 && ri < a.G;
        okb[t] = rj >= 0 && rj < a.G;
        offa[t] = (oka[t] ? ri : 0) * a.ld;
        offb[t] = (okb[t] ? rj : 0) * a.ld;
    }
    dv_f32x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (dv_f32x4){0.f, 0.f, 0.f, 0.f};

    const int full = a.dim / 32 * 32;                 // ascending k-steps of 32 columns: the whole ones, then the partial one
    int k0 = 0;
    for (; k0 + 64 <= full; k0 += 64) {               // two k-steps a trip: the loads of both are issued before the first MFMA
        dv_f16x8 av[2][2], bv[2][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                av[s][t] = dv_load_full<F16, VEC>(a.rows, offa[t], k0 + s * 32 + grp * 8);
                bv[s][t] = dv_load_full<F16, VEC>(a.rows, offb[t], k0 + s * 32 + grp * 8);
            }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[s][x], bv[s][y], acc[x][y], 0, 0, 0);
    }
    if (k0 < full) {
        const int k = k0 + grp * 8;
        dv_f16x8 av[2], bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            av[t] = dv_load_full<F16, VEC>(a.rows, offa[t], k);
            bv[t] = dv_load_full<F16, VEC>(a.rows, offb[t], k);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[x], bv[y], acc[x][y], 0, 0, 0);
    }
    if (full < a.dim) {
        const int k = full + grp * 8;
        dv_f16x8 av[2], bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            av[t] = dv_load_tail<F16>(a.rows, offa[t], k, a.dim);
            bv[t] = dv_load_tail<F16>(a.rows, offb[t], k, a.dim);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[x], bv[y], acc[x][y], 0, 0, 0);
    }

    // C layout: column (B side) = lane & 15, row (A side) = 4 * (lane >> 4) + register.  Whether an A-side slot holds a row is
    // known to the lane that loaded it: one ballot per tile hands it to the lanes that store it.
    const bool diag = ti == tj && wi == wj;
    float* out = a.out + q * a.L * (i64)a.L;
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const unsigned rows_ok = (unsigned)(__ballot(oka[x]) & 0xffffu);
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int j = jbase + y * 16 + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = grp * 4 + r, i = ibase + x * 16 + li;
                if (i >= a.L || j >= a.L || (diag && i > j)) continue;
                const float v = (((rows_ok >> li) & 1u) && okb[y]) ? acc[x][y][r] : 0.f;
                out[(i64)i * a.L + j] = v;
                if (i != j) out[(i64)j * a.L + i] = v;
            }
        }
    }
}

struct DvSelectArgs {
    const float* rel;     // [Q][L]
    const i64* idx;       // [Q][L]
    const float* gram;    // [Q][L][L]
    int L, k;
    float lam, oml, dedup;
    int use_dedup;
    i64 idx_offset;
    float* out_val;       // [Q][k]
    i64* out_idx;         // [Q][k]
    float* out_mmr;       // [Q][k] or null
    int* out_count;       // [Q] or null
};

// fp32(lam * rel) - fp32(oml * m): two roundings of the products, one of the difference, never a fused multiply-add.  The library
// is built with -ffp-contract=fast, under which the backend fuses a product into the subtraction whatever the pragma says, so the
// rounded products also pass through an empty asm statement: the subtraction then sees two values it knows nothing about.
__device__ __forceinline__ float dv_value(float lam, float oml, float rel, float m) {
#pragma clang fp contract(off)
    float a = lam * rel;
    float b = oml * m;
    asm volatile("" : "+v"(a), "+v"(b));
    return a - b;
}

// the better of two (value, position) keys: the greater value, ties to the lower position; INT_MAX is "no eligible slot"
__device__ __forceinline__ void dv_better(float& v, int& p, float v2, int p2) {
    if (v2 > v || (v2 == v && p2 < p)) { v = v2; p = p2; }
}

__global__ __launch_bounds__(DV_MAX_L) void k_mmr_select(DvSelectArgs a) {
    __shared__ float wv[2][DV_MAX_L / 64];
    __shared__ int wp[2][DV_MAX_L / 64];
    const int p = threadIdx.x, lane = p & 63, wave = p >> 6, nw = blockDim.x >> 6;
    const i64 q = blockIdx.x;
    const i64 row = p < a.L ? a.idx[q * a.L + p] : -1;
    const bool has = row >= 0;
    const float rel = has ? a.rel[q * a.L + p] : 0.f;
    const float* gram = a.gram + q * a.L * (i64)a.L;
    float m = 0.f;
    bool picked = false;
    int count = 0;
    for (int t = 0; t < a.k; ++t) {
        const bool elig = has && !picked && (!a.use_dedup || m < a.dedup);
        float v = dv_value(a.lam, a.oml, rel, m);
        if (v != v) v = -INFINITY;                                          // a NaN value counts as -inf
        float bv = elig ? v : -INFINITY;
        int bp = elig ? p : INT_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o, 64);
            const int p2 = __shfl_xor(bp, o, 64);
            dv_better(bv, bp, v2, p2);
        }
        if (nw > 1) {                                                       // the buffers alternate: one barrier per pick
            if (lane == 0) { wv[t & 1][wave] = bv; wp[t & 1][wave] = bp; }
            __syncthreads();
            bv = wv[t & 1][0];
            bp = wp[t & 1][0];
            for (int w = 1; w < nw; ++w) dv_better(bv, bp, wv[t & 1][w], wp[t & 1][w]);
        }
        if (bp == INT_MAX) break;                                           // the same in every thread: nothing is eligible
        if (p == bp) {
            picked = true;
            a.out_val[q * a.k + t] = rel;
            a.out_idx[q * a.k + t] = row + a.idx_offset;
            if (a.out_mmr) a.out_mmr[q * a.k + t] = v;
        }
        if (p < a.L) {
            const float s = gram[(i64)bp * a.L + p];
            if (s > m) m = s;
        }
        ++count;
    }
    for (int t = count + p; t < a.k; t += blockDim.x) {
        a.out_val[q * a.k + t] = -INFINITY;
        a.out_idx[q * a.k + t] = -1;
        if (a.out_mmr) a.out_mmr[q * a.k + t] = -INFINITY;
    }
    if (p == 0 && a.out_count) a.out_count[q] = count;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_shortlist_gram(const void* rows, int rows_dtype, int64_t ld, int64_t G, int dim, const int64_t* idx, int64_t Q, int L,
                         float* out, void* stream) {
    const char* who = "shortlist_gram";
    MI355_REQUIRE(rows && idx && out, "%s: null rows/idx/out pointer", who);
    MI355_REQUIRE(rows_dtype == MI355_DTYPE_F32 || rows_dtype == MI355_DTYPE_F16, "%s: unknown rows dtype %d", who, rows_dtype);
    const bool f16 = rows_dtype == MI355_DTYPE_F16;
    MI355_REQUIRE(G >= 1 && G <= INT_MAX, "%s: G=%lld outside [1, 2^31)", who, (long long)G);
    MI355_REQUIRE(dim >= 1 && dim <= DV_MAX_DIM, "%s: dim=%d outside [1, %d]", who, dim, DV_MAX_DIM);
    MI355_REQUIRE(ld >= dim && ld <= INT_MAX, "%s: ld=%lld outside [dim=%d, 2^31)", who, (long long)ld, dim);
    MI355_REQUIRE(Q >= 0 && Q <= INT_MAX, "%s: Q=%lld outside [0, 2^31)", who, (long long)Q);
    MI355_REQUIRE(L >= 1 && L <= DV_MAX_L, "%s: shortlist length L=%d outside [1, %d]", who, L, DV_MAX_L);
    if (f16) MI355_REQUIRE(((uintptr_t)rows & 15) == 0 && ld % 8 == 0, "%s: fp16 rows must be 16-byte aligned with ld=%lld a multiple "
                           "of 8", who, (long long)ld);
    else MI355_REQUIRE(((uintptr_t)rows & 3) == 0, "%s: fp32 rows must be 4-byte aligned", who);
    MI355_REQUIRE(((uintptr_t)idx & 7) == 0 && ((uintptr_t)out & 3) == 0, "%s: idx must be 8-byte and out 4-byte aligned", who);
    if (Q == 0) return OK;
    RoctxRange range("diversify/shortlist gram");
    const int nt = (L + DV_TILE - 1) / DV_TILE;
    const dim3 grid((unsigned)Q, (unsigned)(nt * (nt + 1) / 2));
    const DvGramArgs a{rows, (i64)ld, (i64)G, dim, (const i64*)idx, L, out};
    const bool vec = ld % 4 == 0 && ((uintptr_t)rows & 15) == 0;            // every row of an fp32 buffer starts on 16 bytes
    hipStream_t st = (hipStream_t)stream;
    if (f16) hipLaunchKernelGGL((k_shortlist_gram<true, true>), grid, dim3(DV_THREADS), 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_shortlist_gram<false, true>), grid, dim3(DV_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_shortlist_gram<false, false>), grid, dim3(DV_THREADS), 0, st, a);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_mmr_select(const float* rel, const int64_t* idx, const float* gram, int64_t Q, int L, int k, float lam, float dedup_or_nan,
                     int64_t idx_offset, float* out_val, int64_t* out_idx, float* out_mmr, int32_t* out_count, void* stream) {
    const char* who = "mmr_select";
    MI355_REQUIRE(rel && idx && gram && out_val && out_idx, "%s: null rel/idx/gram/out_val/out_idx pointer", who);
    MI355_REQUIRE(Q >= 0 && Q <= INT_MAX, "%s: Q=%lld outside [0, 2^31)", who, (long long)Q);
    MI355_REQUIRE(L >= 1 && L <= DV_MAX_L, "%s: shortlist length L=%d outside [1, %d]", who, L, DV_MAX_L);
    MI355_REQUIRE(k >= 1 && k <= L, "%s: k=%d outside [1, L=%d]", who, k, L);
    MI355_REQUIRE(lam >= 0.f && lam <= 1.f, "%s: lam=%g is not a finite float in [0, 1]", who, (double)lam);
    MI355_REQUIRE(!isinf(dedup_or_nan), "%s: dedup=%g must be finite (NaN: no threshold)", who, (double)dedup_or_nan);
    MI355_REQUIRE(((uintptr_t)idx & 7) == 0 && ((uintptr_t)out_idx & 7) == 0, "%s: idx and out_idx must be 8-byte aligned", who);
    if (Q == 0) return OK;
    RoctxRange range("diversify/mmr select");
    const bool use_dedup = !isnan(dedup_or_nan);
    const DvSelectArgs a{rel, (const i64*)idx, gram, L, k, lam, 1.0f - lam, use_dedup ? dedup_or_nan : 0.f, use_dedup ? 1 : 0,
                         (i64)idx_offset, out_val, (i64*)out_idx, out_mmr, out_count};
    const int threads = (L + 63) / 64 * 64;
    hipLaunchKernelGGL(k_mmr_select, dim3((unsigned)Q), dim3(threads), 0, (hipStream_t)stream, a);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
