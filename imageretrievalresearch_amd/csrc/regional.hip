// Regional MaxSim re-ranking (Razavian et al. 2016; Tolias et al., ICLR 2016, section 5; "late interaction"): every query
// region against its best region of a candidate image, the maxima summed with the query's weights.  include/mi355_retrieval.h
// states the score.
//   mi355_region_scores ... one workgroup per (query, slice of its candidate list), one wave per candidate.  The query's fp16
//                           codes are the resident operand: staged into LDS once per workgroup (rows 16 bytes apart in the
//                           banks), or, where Rq_pad rows of ld do not fit the LDS cap, one chunk of d at a time with the
//                           accumulators kept in registers across the chunks.  A candidate's R x ld codes are read from global
//                           memory once, 16 bytes per lane straight into the A operand of v_mfma_f32_16x16x32_f16: lane
//                           (c = lane & 15, g = lane >> 4) of k-step s holds elements 32 s + 8 g .. + 7 of gallery region c, so
//                           the two steps of a 128-byte segment read it whole.  The B operand is the same 16 bytes of query
//                           region c from LDS.  The C tile has the query region on the lane (c) and the gallery regions in
//                           the four registers of the four lane groups: the maximum and its lowest region are taken in
//                           registers, then across the groups by two xor shuffles; the weighted sum runs over the query
//                           regions in ascending order through readlane.
// The k-steps of a pair always run in ascending d, whatever the chunking, the slice or the slot: a pair's bits depend on the
// query's codes, its weights and the row alone.  Pad rows of either operand never reach the maximum or the sum: a gallery pad row
// re-reads the candidate's last region (never out of bounds) and is left out of the maximum by its index; a query pad row is zero
// in LDS and left out of the sum by its index.  No atomics, no host sync, ordinary vector stores.  gfx950 only.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef long long i64;
typedef _Float16 rg_f16x8 __attribute__((ext_vector_type(8)));
typedef float rg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RG_THREADS = 256, RG_WAVES = RG_THREADS / 64;
constexpr int RG_MAX_REGIONS = MI355_REGION_MAX_REGIONS, RG_MAX_L = 1024, RG_MAX_DIM = 65536;
constexpr int RG_SEG = 64;                       // halfs of a 128-byte segment: two k-steps of 32
constexpr int RG_ROW_PAD = 8;                    // halfs between the LDS rows' bank phases (16 bytes)
constexpr size_t RG_LDS_CAP = 64u * 1024u;       // of one workgroup: two or three of them share a CU's 160 KiB
constexpr int RG_TARGET_GROUPS = 1024;           // workgroups a launch aims at when it slices the candidate lists

static inline int rg_pad16(int r) { return (r + 15) / 16 * 16; }
static inline bool rg_shape_ok(int Rq, int dim) { return Rq >= 1 && Rq <= RG_MAX_REGIONS && dim >= 1 && dim <= RG_MAX_DIM; }
static inline int rg_ld(int dim) { return (dim + RG_SEG - 1) / RG_SEG * RG_SEG; }
// halfs of d a workgroup keeps in LDS at a time: the whole row when Rq_pad of them fit the cap, else the largest whole number of
// segments that does (at least one: 64 rows of one segment are 9 KiB)
static inline int rg_chunk(int Rq, int ld) {
    const size_t rows = (size_t)rg_pad16(Rq);
    if (rows * (size_t)(ld + RG_ROW_PAD) * 2 <= RG_LDS_CAP) return ld;
    const size_t halfs = RG_LDS_CAP / (rows * 2) - RG_ROW_PAD;
    return (int)(halfs / RG_SEG * RG_SEG);
}
static inline size_t rg_lds(int Rq, int ld) { return (size_t)rg_pad16(Rq) * (size_t)(rg_chunk(Rq, ld) + RG_ROW_PAD) * 2; }

struct RgArgs {
    const _Float16* q;    // [Q][Rq][ld]
    const _Float16* g;    // [rows][R][ld]
    const i64* idx;       // [Q][L] local rows, or null: slot p is row p
    const float* w;       // [Q][Rq], or null: every weight is `unit`
    float unit;           // fp32(1) / fp32(Rq)
    float* scores;        // [Q][L]
    int* matches;         // [Q][L][Rq], or null
    i64 rows, L;
    int Rq, R, ld, chunk, per_group;   // per_group: slots of a workgroup's slice, a multiple of RG_WAVES
};

// TQ / TG: 16-row tiles of the query / of the gallery regions
template <int TQ, int TG>
__global__ __launch_bounds__(RG_THREADS) void k_region_scores(RgArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_smem[];
    _Float16* qs = reinterpret_cast<_Float16*>(rg_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, grp = lane >> 4;
    const i64 q = blockIdx.x;
    const int lds_ld = a.chunk + RG_ROW_PAD;
    const int nchunks = (a.ld + a.chunk - 1) / a.chunk;
    const i64 s0 = (i64)blockIdx.y * a.per_group;
    const i64 s1 = s0 + a.per_group < a.L ? s0 + a.per_group : a.L;
    const _Float16* qrow = a.q + q * a.Rq * (i64)a.ld;

    // the weights of this lane's query regions (lane c of every group holds region 16 t + c)
    float wl[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        const int i = t * 16 + c;
        wl[t] = i < a.Rq ? (a.w ? a.w[q * a.Rq + i] : a.unit) : 0.f;
    }

    for (i64 b0 = s0; b0 < s1; b0 += RG_WAVES) {                            // the same trips in every wave: barriers inside
        const i64 slot = b0 + wave;
        i64 row = -1;
        if (slot < s1) {
            row = a.idx ? a.idx[q * a.L + slot] : slot;
            if (row < 0 || row >= a.rows) row = -1;                         // a pad, or an index outside the gallery
        }
        const _Float16* gl[TG];                                             // this lane's gallery regions, pad rows clamped
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            const int j = t * 16 + c;
            gl[t] = a.g + ((row < 0 ? 0 : row) * a.R + (j < a.R ? j : a.R - 1)) * (i64)a.ld + grp * 8;
        }
        rg_f32x4 acc[TQ][TG];
#pragma unroll
        for (int tq = 0; tq < TQ; ++tq)
#pragma unroll
            for (int tg = 0; tg < TG; ++tg) acc[tq][tg] = (rg_f32x4){0.f, 0.f, 0.f, 0.f};

        for (int ch = 0; ch < nchunks; ++ch) {
            const int k0 = ch * a.chunk;
            const int kn = a.ld - k0 < a.chunk ? a.ld - k0 : a.chunk;      // a multiple of RG_SEG
            if (nchunks > 1 || b0 == s0) {                                  // the resident query: staged once per workgroup
                if (nchunks > 1) __syncthreads();                          // nobody still reads the chunk before
                const int units = kn / 8;                                   // 16-byte units of a row's chunk
                for (int e = tid; e < TQ * 16 * units; e += RG_THREADS) {
                    const int i = e / units, u = e - i * units;
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if (i < a.Rq) v = *reinterpret_cast<const uint4*>(qrow + (i64)i * a.ld + k0 + u * 8);
                    *reinterpret_cast<uint4*>(qs + (size_t)i * lds_ld + u * 8) = v;
                }
                __syncthreads();
            }
            if (row >= 0) {
                const _Float16* ql = qs + (size_t)c * lds_ld + grp * 8;
#pragma unroll 2
                for (int k = 0; k < kn; k += RG_SEG) {
                    rg_f16x8 av[2][TG], bv[2][TQ];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
#pragma unroll
                        for (int t = 0; t < TG; ++t) av[s][t] = *reinterpret_cast<const rg_f16x8*>(gl[t] + k0 + k + s * 32);
#pragma unroll
                        for (int t = 0; t < TQ; ++t)
                            bv[s][t] = *reinterpret_cast<const rg_f16x8*>(ql + (size_t)t * 16 * lds_ld + k + s * 32);
                    }
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int tq = 0; tq < TQ; ++tq)
#pragma unroll
                            for (int tg = 0; tg < TG; ++tg)
                                acc[tq][tg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[s][tg], bv[s][tq], acc[tq][tg], 0, 0, 0);
                }
            }
        }
        if (slot >= s1) continue;
        // C layout: column (query region) = lane & 15, row (gallery region) = 4 * (lane >> 4) + register
        float score = 0.f;
#pragma unroll
        for (int tq = 0; tq < TQ; ++tq) {
            float m = 0.f;
            int at = -1;
            if (row >= 0) {
#pragma unroll
                for (int tg = 0; tg < TG; ++tg)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = tg * 16 + grp * 4 + r;
                        const float v = acc[tq][tg][r];
                        if (j < a.R && (at < 0 || v > m)) { m = v; at = j; }
                    }
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {                        // the other lane groups: the larger, ties to the lower region
                    const float m2 = __shfl_xor(m, o, 64);
                    const int at2 = __shfl_xor(at, o, 64);
                    if (at2 >= 0 && (at < 0 || m2 > m || (m2 == m && at2 < at))) { m = m2; at = at2; }
                }
            }
            const int i = tq * 16 + c;
            if (a.matches && grp == 0 && i < a.Rq) a.matches[(q * a.L + slot) * a.Rq + i] = at;
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) {                               // ascending query region, the same in every lane
                const float mi = __shfl(m, cc, 64), wi = __shfl(wl[tq], cc, 64);
                if (tq * 16 + cc < a.Rq) score += wi * mi;
            }
        }
        if (lane == 0) a.scores[q * a.L + slot] = row >= 0 ? score : -INFINITY;
    }
}

typedef void (*RgKernel)(RgArgs);
template <int TQ>
static RgKernel rg_kernel_tg(int tg) {
    switch (tg) {
        case 1: return k_region_scores<TQ, 1>;
        case 2: return k_region_scores<TQ, 2>;
        case 3: return k_region_scores<TQ, 3>;
        default: return k_region_scores<TQ, 4>;
    }
}
static RgKernel rg_kernel(int tq, int tg) {
    switch (tq) {
        case 1: return rg_kernel_tg<1>(tg);
        case 2: return rg_kernel_tg<2>(tg);
        case 3: return rg_kernel_tg<3>(tg);
        default: return rg_kernel_tg<4>(tg);
    }
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_region_scores_lds_bytes(int Rq, int dim) { return rg_shape_ok(Rq, dim) ? rg_lds(Rq, rg_ld(dim)) : 0; }

int mi355_region_scores(const void* qcodes, int64_t Q, int Rq, const void* gcodes, int64_t rows, int R, int dim, int ld,
                        const int64_t* idx, int64_t L, const float* weights, float* out_scores, int32_t* out_matches, void* stream) {
    const char* who = "region_scores";
    MI355_REQUIRE(qcodes && gcodes && out_scores, "%s: null qcodes/gcodes/out_scores pointer", who);
    MI355_REQUIRE(Q >= 0 && Q <= INT_MAX, "%s: Q=%lld outside [0, 2^31)", who, (long long)Q);
    MI355_REQUIRE(Rq >= 1 && Rq <= RG_MAX_REGIONS, "%s: Rq=%d outside [1, %d]", who, Rq, RG_MAX_REGIONS);
    MI355_REQUIRE(R >= 1 && R <= RG_MAX_REGIONS, "%s: R=%d outside [1, %d]", who, R, RG_MAX_REGIONS);
    MI355_REQUIRE(rows >= 1 && rows <= INT_MAX, "%s: rows=%lld outside [1, 2^31)", who, (long long)rows);
    MI355_REQUIRE(dim >= 1 && dim <= RG_MAX_DIM, "%s: dim=%d outside [1, %d]", who, dim, RG_MAX_DIM);
    MI355_REQUIRE(ld == rg_ld(dim), "%s: ld=%d is not dim=%d rounded up to a multiple of %d", who, ld, dim, RG_SEG);
    if (idx) MI355_REQUIRE(L >= 1 && L <= RG_MAX_L, "%s: list length L=%lld outside [1, %d]", who, (long long)L, RG_MAX_L);
    else MI355_REQUIRE(L == rows, "%s: without idx every row is scored: L=%lld must be rows=%lld", who, (long long)L, (long long)rows);
    MI355_REQUIRE((((uintptr_t)qcodes | (uintptr_t)gcodes) & 15) == 0, "%s: qcodes and gcodes must be 16-byte aligned", who);
    const size_t lds = mi355_region_scores_lds_bytes(Rq, dim);
    MI355_REQUIRE(lds > 0 && lds <= RG_LDS_CAP, "%s: %zu bytes of LDS for Rq=%d dim=%d", who, lds, Rq, dim);
    if (Q == 0) return OK;
    RoctxRange range("regional/scores");
    const int tq = rg_pad16(Rq) / 16, tg = rg_pad16(R) / 16;
    RgKernel kern = rg_kernel(tq, tg);
    // up to 64 KiB of dynamic LDS: raise each kernel's limit once per device (as diffusion.hip does)
    static bool raised[4][4][MI355_MAX_DEVICES] = {};
    if (first_time_on_this_device(raised[tq - 1][tg - 1]))
        MI355_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RG_LDS_CAP));
    // slices of a list: enough workgroups to fill the device, each of whole rounds of its waves
    i64 slices = (RG_TARGET_GROUPS + Q - 1) / Q;
    const i64 rounds = (L + RG_WAVES - 1) / RG_WAVES;
    if (slices > rounds) slices = rounds;
    if (slices > 65535) slices = 65535;
    const i64 per_group = (rounds + slices - 1) / slices * RG_WAVES;
    MI355_REQUIRE(per_group <= INT_MAX, "%s: rows=%lld too many for one launch", who, (long long)rows);
    slices = (L + per_group - 1) / per_group;
    RgArgs a{(const _Float16*)qcodes, (const _Float16*)gcodes, (const i64*)idx, weights, 1.0f / (float)Rq, out_scores, out_matches,
             (i64)rows, (i64)L, Rq, R, ld, rg_chunk(Rq, ld), (int)per_group};
    hipLaunchKernelGGL(kern, dim3((unsigned)Q, (unsigned)slices), dim3(RG_THREADS), lds, (hipStream_t)stream, a);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
