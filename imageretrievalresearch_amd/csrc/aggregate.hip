// Feature-map aggregation: SPoC / MAC / R-MAC (Tolias et al., ICLR 2016), GeM (Radenovic et al., TPAMI 2018) and CroW (Kalantidis
// et al., ECCV 2016) descriptors of a backbone's last map.  include/mi355_retrieval.h states the arithmetic; in short, for a map
// fm [B][C][H][W] fp32 and regions (y0, x0, h, w) inside it:
//   regional value v[b][r][c]: mean = sum / (h w);  max = the maximum, exact;
//                              gem  = m * (mean((t/m)^p))^(1/p), t = max(x, eps_clamp), m = max t  (p scalar or per channel)
//   normalize:  v[b][r][:] /= max(|v[b][r][:]|_2, eps);  then the vectors themselves [B][R][C], or their sum over r in region order,
//   divided again by max(its norm, eps).
//   CroW: X' = max(X, 0), S = sum_c X', St = sqrt(S / sqrt(sum_hw S^2)) (0 for an all-zero S), F_c = sum_hw St X'_c, Q_c = share of
//   positions with X_c > 0, I_c = log(sum Q / Q_c) (0 for Q_c = 0), descriptor I * F, normalised the same way.
//
//   k_agg_pool ....... one pass over the map.  The work is cut into slabs of CS channels of one image (CS a rule of (C, H W)
//                      alone: about 4 KB of map, at least 64 slabs per image where C allows); a workgroup walks groups of G
//                      consecutive slabs (G = 1 at small B, up to 8 where there is work enough: a launch choice) blockIdx.x,
//                      blockIdx.x + gridDim.x, ...  A group is contiguous in memory whatever H W is, so it is loaded
//                      as the flat array it is - scalar loads up to the first 16-byte boundary, float4 loads, a scalar tail -
//                      and each value is put into its channel's LDS row (row stride H W | 1: odd, so that threads that walk
//                      different channels hit different banks).  Every (channel, region) pair is then one task of LPT lanes
//                      (1, 4, 16 or 64, by the slab's task count; the lanes take the columns of a region's row, or stride a
//                      full-width region as the one run it is) that pools the region from LDS: R-MAC reads the map from HBM
//                      once, not once per region.  The pooled values go to the workspace with one partial sum of squares per
//                      (image, region, slab).
//   k_agg_finish ..... one workgroup per image: the partial sums of squares in slab order, the regional norms, the sum over the
//                      regions in region order and the last norm.
//   k_crow_partial / k_crow_weights / k_agg_pool (CroW flavour) / k_crow_finish: S by channel slab and position tile, St per
//                      image, F and Q per channel slab through the same LDS staging, then I * F and the norm.
// Every sum has a fixed order: per lane in element order, across the lanes of a task or wave by xor shuffles, across waves and
// slabs in index order.  Which workgroup handles a slab changes with B; what a slab computes does not.  No global atomics; no
// workgroup waits on another; every loop is bounded before it starts.  gfx950 only.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef long long i64;

constexpr int AG_THREADS = 256, AG_WAVES = AG_THREADS / 64;
constexpr int AG_MAX_SIDE = MI355_AGG_MAX_SIDE, AG_MAX_R = MI355_AGG_MAX_REGIONS, AG_MAX_HW = AG_MAX_SIDE * AG_MAX_SIDE;
constexpr int AG_SLAB_FLOATS = 4096, AG_SLAB_MIN_FLOATS = 1024, AG_MAX_CS = 128, AG_WANT_SLABS = 64;
constexpr int AG_MAX_B = 1 << 22;                      // B x 16 position tiles x 32 slabs is a grid's x extent
constexpr int AG_MAX_GROUP = 8, AG_GROUP_LDS = 48 * 1024;
constexpr int AG_MAX_GRID = 2048;                      // workgroups of the pooling launch: 8 per CU
constexpr int AG_CROW = 3;                             // the pooling kernel's fourth flavour (after MI355_AGG_MEAN / MAX / GEM)
constexpr int AG_CROW_SLABS = 32;
constexpr float AG_P_MIN = 0.0009765625f, AG_P_MAX = 64.f;

// the region table travels in the kernel arguments: y0 | x0 << 8 | h << 16 | w << 24
struct AggRegions {
    unsigned packed[AG_MAX_R];
};

struct AggPlan {
    int CS, nslab, HWP, lpt;
    int G, ngroup;                                     // slabs a workgroup stages at once (a launch choice), groups per image
    unsigned magic;                                    // i / HW = umulhi(i, magic) for i < 2^20 (HW > 1)
};
static AggPlan agg_plan(int C, int HW, int R) {
    AggPlan p{};
    int CS = AG_SLAB_FLOATS / HW;
    CS = CS < 1 ? 1 : CS > AG_MAX_CS ? AG_MAX_CS : CS;
    if (CS > C) CS = C;
    while (CS > 1 && cdiv(C, CS) < AG_WANT_SLABS && CS * HW > AG_SLAB_MIN_FLOATS) CS /= 2;
    p.CS = CS;
    p.nslab = cdiv(C, CS);
    p.HWP = HW | 1;
    // lanes per (channel, region) task: as many as keep the slab's tasks within a few rounds of the 256 threads - a whole-map
    // pool (R = 1) has few tasks and long regions, a 30-region grid on a 7 x 7 map the opposite
    const long tasks = (long)CS * R;
    p.lpt = tasks * 64 <= 512 ? 64 : tasks * 16 <= 512 ? 16 : tasks * 4 <= 2048 ? 4 : 1;
    if (HW > 64 && p.lpt < 16) p.lpt = 16;
    p.magic = HW > 1 ? (unsigned)((1ull << 32) / (unsigned)HW) + 1u : 0u;
    return p;
}
static int crow_slabs(int C, int HW) {
    i64 n = 2 * (i64)C / HW;
    n = n < 1 ? 1 : n > AG_CROW_SLABS ? AG_CROW_SLABS : n;
    return (int)(n > C ? C : n);
}

struct AggPoolArgs {
    const float* fm;
    i64 B;
    int C, HW, W, R;
    AggPlan plan;
    float p;
    const float* pvec;     // [C] or null
    float eps_clamp;
    const float* wts;      // CroW: St [B][HW]
    float* vals;           // [B][R][C]
    float* ssq;            // [B][R][nslab], or null (CroW, or nothing to normalise)
    float* q;              // CroW: Q [B][C]
};

template <int LPT>
__device__ __forceinline__ float grp_sum(float v) {
#pragma unroll
    for (int o = LPT / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int LPT>
__device__ __forceinline__ float grp_max(float v) {
#pragma unroll
    for (int o = LPT / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The sum of v over the workgroup, the same bits in every thread: lanes by xor shuffles, waves in order.
__device__ __forceinline__ float ag_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                   // whoever still reads red from the sum before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < AG_WAVES; ++w) s += red[w];
    return s;
}

template <int LPT, int KIND>
__global__ __launch_bounds__(AG_THREADS) void k_agg_pool(AggPoolArgs a, AggRegions rg) {
    extern __shared__ __attribute__((aligned(16))) float ag_smem[];
    const int tid = threadIdx.x, HW = a.HW, HWP = a.plan.HWP, CS = a.plan.CS, R = a.R;
    const int GCS = a.plan.G * CS;                     // the channels of a group of G consecutive slabs
    float* stage = ag_smem;                            // [GCS][HWP]
    float* pooled = stage + GCS * HWP;                 // [R][GCS]
    float* wts = pooled + R * GCS;                     // CroW: [HW]
    constexpr int TPB = AG_THREADS / LPT;
    const int grp = tid / LPT, gl = tid % LPT;
    const unsigned nwork = (unsigned)a.B * (unsigned)a.plan.ngroup;         // below 2^31: checked on the host
    for (unsigned s = blockIdx.x; s < nwork; s += gridDim.x) {
        const unsigned bu = s / (unsigned)a.plan.ngroup;
        const i64 b = bu;
        const int sl0 = (int)(s - bu * (unsigned)a.plan.ngroup) * a.plan.G;
        const int c0 = sl0 * CS, cn = min(GCS, a.C - c0), n = cn * HW;
        const float* src = a.fm + (b * a.C + c0) * HW;
        // the group as a flat array: scalar head up to 16-byte alignment, float4 body, scalar tail
        const int head = min(n, (int)((4u - (unsigned)(((uintptr_t)src >> 2) & 3u)) & 3u));
        const int nvec = (n - head) >> 2;
        auto put = [&](int i, float v) {
            const int ch = HW > 1 ? (int)__umulhi((unsigned)i, a.plan.magic) : i;
            stage[ch * HWP + (i - ch * HW)] = v;
        };
        if (tid < head) put(tid, src[tid]);
        const float4* src4 = reinterpret_cast<const float4*>(src + head);
        for (int v = tid; v < nvec; v += AG_THREADS) {
            const float4 x = src4[v];
            const int i = head + 4 * v;
            put(i, x.x); put(i + 1, x.y); put(i + 2, x.z); put(i + 3, x.w);
        }
        {
            const int i = head + 4 * nvec + tid;
            if (i < n) put(i, src[i]);
        }
        if constexpr (KIND == AG_CROW)
            for (int i = tid; i < HW; i += AG_THREADS) wts[i] = a.wts[b * HW + i];
        __syncthreads();

        const int ntask = cn * R;
        for (int t0 = 0; t0 < ntask; t0 += TPB) {
            const int t = t0 + grp;
            const bool live = t < ntask;
            const int r = live ? t / cn : 0, cl = live ? t - r * cn : 0;
            const unsigned pk = rg.packed[r];
            const int y0 = pk & 255u, x0 = (pk >> 8) & 255u;
            int h = (pk >> 16) & 255u, w = pk >> 24;
            const float* row = stage + cl * HWP + y0 * a.W + x0;
            const float count = (float)(h * w);
            if (w == a.W) {                            // rows of the full width are one run of h w values
                w *= h;
                h = 1;
            }
            float val = 0.f;
            if constexpr (KIND == MI355_AGG_MEAN) {
                float acc = 0.f;
                for (int y = 0; y < h; ++y)
#pragma unroll 4
                    for (int x = gl; x < w; x += LPT) acc += row[y * a.W + x];
                val = grp_sum<LPT>(acc) / count;
            } else if constexpr (KIND == MI355_AGG_MAX) {
                float m = -INFINITY;
                for (int y = 0; y < h; ++y)
#pragma unroll 4
                    for (int x = gl; x < w; x += LPT) m = fmaxf(m, row[y * a.W + x]);
                val = grp_max<LPT>(m);
            } else if constexpr (KIND == MI355_AGG_GEM) {
                float pc = a.pvec ? a.pvec[c0 + cl] : a.p;
                pc = fminf(fmaxf(pc, AG_P_MIN), AG_P_MAX);                  // also a NaN of the per-channel tensor
                float m = 0.f;                                              // every t is >= eps_clamp > 0
                for (int y = 0; y < h; ++y)
#pragma unroll 4
                    for (int x = gl; x < w; x += LPT) m = fmaxf(m, fmaxf(row[y * a.W + x], a.eps_clamp));
                m = grp_max<LPT>(m);
                float acc = 0.f;
                for (int y = 0; y < h; ++y)
#pragma unroll 4
                    for (int x = gl; x < w; x += LPT) acc += exp2f(pc * log2f(fmaxf(row[y * a.W + x], a.eps_clamp) / m));
                const float mean = grp_sum<LPT>(acc) / count;               // in [1 / (h w), 1]
                val = m * exp2f(log2f(mean) / pc);
            } else {
                float acc = 0.f, cnt = 0.f;
#pragma unroll 4
                for (int i = gl; i < HW; i += LPT) {
                    const float x = stage[cl * HWP + i];
                    acc += wts[i] * fmaxf(x, 0.f);
                    cnt += x > 0.f ? 1.f : 0.f;
                }
                val = grp_sum<LPT>(acc);
                cnt = grp_sum<LPT>(cnt);
                if (live && gl == 0) a.q[b * a.C + c0 + cl] = cnt / (float)HW;
            }
            if (live && gl == 0) {
                pooled[r * GCS + cl] = val;
                a.vals[(b * R + r) * a.C + c0 + cl] = val;
            }
        }
        __syncthreads();
        // each slab's share of every regional vector's sum of squares: one wave per (region, slab), lanes stride the slab's
        // channels - the same sum whichever group the slab is staged with
        if (a.ssq) {
            const int nsl = (cn + CS - 1) / CS;
            for (int pi = tid >> 6; pi < R * nsl; pi += AG_WAVES) {
                const int r = pi / nsl, j = pi - r * nsl, cj = min(CS, cn - j * CS);
                float acc = 0.f;
                for (int k = tid & 63; k < cj; k += 64) {
                    const float v = pooled[r * GCS + j * CS + k];
                    acc += v * v;
                }
                acc = wave_sum(acc);
                if ((tid & 63) == 0) a.ssq[(b * R + r) * a.plan.nslab + sl0 + j] = acc;
            }
            __syncthreads();                           // pooled is written again by the next group
        }
    }
}

// ---- the second launch
struct AggFinishArgs {
    const float* vals;     // [B][R][C]
    const float* ssq;      // [B][R][nslab], null: the regional vectors are taken as they are
    int R, C, nslab, normalize, return_regions;
    float eps;
    float* out;            // [B][R][C] or [B][C]
};

__global__ __launch_bounds__(AG_THREADS) void k_agg_finish(AggFinishArgs a) {
    __shared__ float div[AG_MAX_R];
    __shared__ float red[AG_WAVES];
    const int tid = threadIdx.x, R = a.R, C = a.C;
    const i64 b = blockIdx.x;
    if (tid < R) {
        float d = 1.f;
        if (a.ssq) {
            const float* p = a.ssq + (b * R + tid) * a.nslab;
            float s = 0.f;
            for (int sl = 0; sl < a.nslab; ++sl) s += p[sl];
            d = fmaxf(sqrtf(s), a.eps);
        }
        div[tid] = d;
    }
    __syncthreads();
    const float* vb = a.vals + b * R * C;
    if (a.return_regions) {
        float* ob = a.out + b * R * C;
        for (int r = 0; r < R; ++r)
            for (int c = tid; c < C; c += AG_THREADS) ob[(i64)r * C + c] = vb[(i64)r * C + c] / div[r];
        return;
    }
    float part = 0.f;
    for (int c = tid; c < C; c += AG_THREADS) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += vb[(i64)r * C + c] / div[r];
        if (!a.normalize) a.out[b * C + c] = s;
        part += s * s;
    }
    if (!a.normalize) return;                                               // the same in every thread
    const float d = fmaxf(sqrtf(ag_block_sum(part, red)), a.eps);
    for (int c = tid; c < C; c += AG_THREADS) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += vb[(i64)r * C + c] / div[r];       // the same bits as above
        a.out[b * C + c] = s / d;
    }
}

// ---- CroW
// S of one channel slab and one tile of PT positions: the workgroup is G = 256 / PT groups of PT lanes, group g adds channels
// g, g + G, ... of the slab in order, the groups are added in order.
__global__ __launch_bounds__(AG_THREADS) void k_crow_partial(const float* fm, int C, int HW, int PT, int tiles, int CS1, int nslab1,
                                                             float* spart) {
    __shared__ float red[AG_THREADS];
    const int tid = threadIdx.x, lane = tid % PT, g = tid / PT, G = AG_THREADS / PT;
    const int per = tiles * nslab1, w = blockIdx.x % per, tile = w % tiles, sl = w / tiles;
    const i64 b = blockIdx.x / per;
    const int hw = tile * PT + lane, c0 = sl * CS1, c1 = min(C, c0 + CS1);
    float acc = 0.f;
    if (hw < HW)
        for (int c = c0 + g; c < c1; c += G) acc += fmaxf(fm[(b * C + c) * HW + hw], 0.f);
    red[tid] = acc;
    __syncthreads();
    if (g == 0 && hw < HW) {
        float s = red[lane];
        for (int k = 1; k < G; ++k) s += red[k * PT + lane];
        spart[(b * nslab1 + sl) * HW + hw] = s;
    }
}

__global__ __launch_bounds__(AG_THREADS) void k_crow_weights(const float* spart, int HW, int nslab1, float* wts) {
    __shared__ float S[AG_MAX_HW];
    __shared__ float red[AG_WAVES];
    const int tid = threadIdx.x;
    const i64 b = blockIdx.x;
    float part = 0.f;
    for (int hw = tid; hw < HW; hw += AG_THREADS) {
        float s = 0.f;
        for (int sl = 0; sl < nslab1; ++sl) s += spart[(b * nslab1 + sl) * HW + hw];
        S[hw] = s;
        part += s * s;
    }
    const float tot = ag_block_sum(part, red);
    const float z = sqrtf(tot);
    for (int hw = tid; hw < HW; hw += AG_THREADS) wts[b * HW + hw] = tot > 0.f ? sqrtf(S[hw] / z) : 0.f;   // its own S
}

__global__ __launch_bounds__(AG_THREADS) void k_crow_finish(const float* F, const float* Q, int C, int normalize, float eps, float* out) {
    __shared__ float red[AG_WAVES];
    const int tid = threadIdx.x;
    const i64 b = blockIdx.x;
    float part = 0.f;
    for (int c = tid; c < C; c += AG_THREADS) part += Q[b * C + c];
    const float qsum = ag_block_sum(part, red);
    part = 0.f;
    for (int c = tid; c < C; c += AG_THREADS) {
        const float q = Q[b * C + c];
        const float v = q > 0.f ? logf(qsum / q) * F[b * C + c] : 0.f;
        if (!normalize) out[b * C + c] = v;
        part += v * v;
    }
    if (!normalize) return;
    const float d = fmaxf(sqrtf(ag_block_sum(part, red)), eps);
    for (int c = tid; c < C; c += AG_THREADS) {
        const float q = Q[b * C + c];
        out[b * C + c] = (q > 0.f ? logf(qsum / q) * F[b * C + c] : 0.f) / d;
    }
}

// ---- host side
static bool agg_shape_ok(i64 B, int C, int R) {
    return B >= 0 && B <= AG_MAX_B && C >= 1 && R >= 1 && R <= AG_MAX_R && (double)B * R * C < 2147483648.0;
}

// The workspace of both entries.  The sizer does not know H W, so every piece is sized for the worst map: one partial sum of
// squares per channel (a slab is at least one channel), 2 C + 4096 partial S values (crow_slabs).
struct AggWs {
    float *vals, *ssq, *q, *wts, *spart;
    size_t total;
};
static AggWs agg_ws(void* ws, i64 B, int C, int R) {
    WsCarver cv(ws);
    AggWs w{};
    w.vals = (float*)cv.take((size_t)B * R * C * sizeof(float));
    w.ssq = (float*)cv.take((size_t)B * R * C * sizeof(float));
    w.q = (float*)cv.take((size_t)B * C * sizeof(float));
    w.wts = (float*)cv.take((size_t)B * AG_MAX_HW * sizeof(float));
    w.spart = (float*)cv.take((size_t)B * (2 * (size_t)C + AG_MAX_HW) * sizeof(float));
    w.total = cv.total();
    return w;
}

static size_t agg_pool_lds(const AggPlan& pl, int G, int R, int HW, bool crow) {
    return ((size_t)G * pl.CS * pl.HWP + (size_t)R * G * pl.CS + (crow ? HW : 0)) * sizeof(float);
}

template <int LPT>
static void agg_pool_launch(int kind, unsigned grid, size_t lds, hipStream_t st, const AggPoolArgs& a, const AggRegions& rg) {
    switch (kind) {
        case MI355_AGG_MEAN: hipLaunchKernelGGL((k_agg_pool<LPT, MI355_AGG_MEAN>), dim3(grid), dim3(AG_THREADS), lds, st, a, rg); break;
        case MI355_AGG_MAX: hipLaunchKernelGGL((k_agg_pool<LPT, MI355_AGG_MAX>), dim3(grid), dim3(AG_THREADS), lds, st, a, rg); break;
        case MI355_AGG_GEM: hipLaunchKernelGGL((k_agg_pool<LPT, MI355_AGG_GEM>), dim3(grid), dim3(AG_THREADS), lds, st, a, rg); break;
        default: hipLaunchKernelGGL((k_agg_pool<LPT, AG_CROW>), dim3(grid), dim3(AG_THREADS), lds, st, a, rg); break;
    }
}
static void agg_pool(int kind, hipStream_t st, AggPoolArgs a, const AggRegions& rg) {
    // A workgroup stages G consecutive slabs of an image at once: 1 while that still gives every workgroup of a full grid a
    // group, up to 8 at large B, where the cost of a trip round the slab loop is what the launch spends most of its time on.
    // Only the launch changes with G (so with B): a slab's sums are the same in every group.
    const bool crow = kind == AG_CROW;
    int G = 1;
    while (G < AG_MAX_GROUP && 2 * G <= a.plan.nslab && a.B * cdiv(a.plan.nslab, 2 * G) >= AG_MAX_GRID &&
           agg_pool_lds(a.plan, 2 * G, a.R, a.HW, crow) <= AG_GROUP_LDS)
        G *= 2;
    a.plan.G = G;
    a.plan.ngroup = cdiv(a.plan.nslab, G);
    const i64 nwork = a.B * a.plan.ngroup;
    const unsigned grid = (unsigned)(nwork < AG_MAX_GRID ? nwork : AG_MAX_GRID);
    const size_t lds = agg_pool_lds(a.plan, G, a.R, a.HW, crow);                        // at most 50 KB: below the default limit
    switch (a.plan.lpt) {
        case 1: agg_pool_launch<1>(kind, grid, lds, st, a, rg); break;
        case 4: agg_pool_launch<4>(kind, grid, lds, st, a, rg); break;
        case 16: agg_pool_launch<16>(kind, grid, lds, st, a, rg); break;
        default: agg_pool_launch<64>(kind, grid, lds, st, a, rg); break;
    }
}

static bool agg_finite_nonneg(float v) { return isfinite(v) && v >= 0.f; }

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_aggregate_workspace_bytes(int64_t B, int C, int R) {
    if (B == 0 || !agg_shape_ok(B, C, R)) return 0;
    return agg_ws(nullptr, B, C, R).total;
}

int mi355_aggregate_regions(const float* fm, int64_t B, int C, int H, int W, const int32_t* regions, int R, int pool, float p,
                            const float* p_channels, float eps_clamp, int normalize, int return_regions, float eps, float* out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "aggregate_regions";
    MI355_REQUIRE(fm && regions && out, "%s: null fm/regions/out pointer", who);
    MI355_REQUIRE(B >= 0 && B <= AG_MAX_B, "%s: B=%lld outside [0, 2^22]", who, (long long)B);
    MI355_REQUIRE(C >= 1, "%s: C=%d must be at least 1", who, C);
    MI355_REQUIRE(H >= 1 && H <= AG_MAX_SIDE, "%s: H=%d outside [1, %d]", who, H, AG_MAX_SIDE);
    MI355_REQUIRE(W >= 1 && W <= AG_MAX_SIDE, "%s: W=%d outside [1, %d]", who, W, AG_MAX_SIDE);
    MI355_REQUIRE(R >= 1 && R <= AG_MAX_R, "%s: R=%d outside [1, %d]", who, R, AG_MAX_R);
    MI355_REQUIRE(pool == MI355_AGG_MEAN || pool == MI355_AGG_MAX || pool == MI355_AGG_GEM, "%s: pool=%d is not mean (0), max (1) or gem (2)",
                  who, pool);
    if (pool == MI355_AGG_GEM) {
        MI355_REQUIRE(p_channels || (isfinite(p) && p > 0.f && p <= AG_P_MAX), "%s: p=%g outside (0, %g]", who, (double)p, (double)AG_P_MAX);
        MI355_REQUIRE(isfinite(eps_clamp) && eps_clamp > 0.f, "%s: eps_clamp=%g must be a finite float above 0", who, (double)eps_clamp);
    }
    MI355_REQUIRE(agg_finite_nonneg(eps), "%s: eps=%g must be a finite float >= 0", who, (double)eps);
    MI355_REQUIRE(agg_shape_ok(B, C, R), "%s: B=%lld x R=%d x C=%d values are too many", who, (long long)B, R, C);
    AggRegions rg{};
    for (int r = 0; r < R; ++r) {
        const int32_t* q = regions + 4 * r;
        MI355_REQUIRE(q[2] >= 1 && q[3] >= 1 && q[0] >= 0 && q[1] >= 0 && q[0] <= H - q[2] && q[1] <= W - q[3],
                      "%s: region %d = (y0=%d, x0=%d, h=%d, w=%d) is empty or outside the %dx%d map", who, r, q[0], q[1], q[2], q[3], H, W);
        rg.packed[r] = (unsigned)q[0] | (unsigned)q[1] << 8 | (unsigned)q[2] << 16 | (unsigned)q[3] << 24;
    }
    if (B == 0) return OK;
    const AggWs ws = agg_ws(workspace, B, C, R);
    MI355_REQUIRE(workspace && workspace_bytes >= ws.total, "%s: workspace of %zu bytes at %p, %zu needed (mi355_aggregate_workspace_bytes)",
                  who, workspace_bytes, workspace, ws.total);
    RoctxRange range("aggregate/regions");
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    AggPoolArgs a{};
    a.fm = fm; a.B = B; a.C = C; a.HW = HW; a.W = W; a.R = R;
    a.plan = agg_plan(C, HW, R);
    a.p = p; a.pvec = pool == MI355_AGG_GEM ? p_channels : nullptr; a.eps_clamp = eps_clamp;
    a.vals = ws.vals; a.ssq = normalize ? ws.ssq : nullptr;
    agg_pool(pool, st, a, rg);
    MI355_LAUNCH_CHECK();
    const AggFinishArgs f{ws.vals, a.ssq, R, C, a.plan.nslab, normalize ? 1 : 0, return_regions ? 1 : 0, eps, out};
    hipLaunchKernelGGL(k_agg_finish, dim3((unsigned)B), dim3(AG_THREADS), 0, st, f);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_aggregate_sum(const float* vecs, int64_t B, int R, int D, int normalize, float eps, float* out, void* stream) {
    const char* who = "aggregate_sum";
    MI355_REQUIRE(vecs && out, "%s: null vecs/out pointer", who);
    MI355_REQUIRE(B >= 0 && B <= AG_MAX_B, "%s: B=%lld outside [0, 2^22]", who, (long long)B);
    MI355_REQUIRE(R >= 1 && R <= AG_MAX_R, "%s: R=%d outside [1, %d]", who, R, AG_MAX_R);
    MI355_REQUIRE(D >= 1, "%s: D=%d must be at least 1", who, D);
    MI355_REQUIRE(agg_finite_nonneg(eps), "%s: eps=%g must be a finite float >= 0", who, (double)eps);
    MI355_REQUIRE(agg_shape_ok(B, D, R), "%s: B=%lld x R=%d x D=%d values are too many", who, (long long)B, R, D);
    if (B == 0) return OK;
    RoctxRange range("aggregate/sum");
    const AggFinishArgs f{vecs, nullptr, R, D, 0, normalize ? 1 : 0, 0, eps, out};
    hipLaunchKernelGGL(k_agg_finish, dim3((unsigned)B), dim3(AG_THREADS), 0, (hipStream_t)stream, f);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_aggregate_crow(const float* fm, int64_t B, int C, int H, int W, int normalize, float eps, float* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
    const char* who = "aggregate_crow";
    MI355_REQUIRE(fm && out, "%s: null fm/out pointer", who);
    MI355_REQUIRE(B >= 0 && B <= AG_MAX_B, "%s: B=%lld outside [0, 2^22]", who, (long long)B);
    MI355_REQUIRE(C >= 1, "%s: C=%d must be at least 1", who, C);
    MI355_REQUIRE(H >= 1 && H <= AG_MAX_SIDE, "%s: H=%d outside [1, %d]", who, H, AG_MAX_SIDE);
    MI355_REQUIRE(W >= 1 && W <= AG_MAX_SIDE, "%s: W=%d outside [1, %d]", who, W, AG_MAX_SIDE);
    MI355_REQUIRE(agg_finite_nonneg(eps), "%s: eps=%g must be a finite float >= 0", who, (double)eps);
    MI355_REQUIRE(agg_shape_ok(B, C, 1), "%s: B=%lld x C=%d values are too many", who, (long long)B, C);
    if (B == 0) return OK;
    const AggWs ws = agg_ws(workspace, B, C, 1);
    MI355_REQUIRE(workspace && workspace_bytes >= ws.total, "%s: workspace of %zu bytes at %p, %zu needed (mi355_aggregate_workspace_bytes)",
                  who, workspace_bytes, workspace, ws.total);
    RoctxRange range("aggregate/crow");
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    int PT = 1;
    while (PT < HW && PT < AG_THREADS) PT <<= 1;
    const int tiles = cdiv(HW, PT), want = crow_slabs(C, HW), CS1 = cdiv(C, want), nslab1 = cdiv(C, CS1);
    hipLaunchKernelGGL(k_crow_partial, dim3((unsigned)(tiles * nslab1 * B)), dim3(AG_THREADS), 0, st, fm, C, HW, PT, tiles, CS1,
                       nslab1, ws.spart);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_crow_weights, dim3((unsigned)B), dim3(AG_THREADS), 0, st, (const float*)ws.spart, HW, nslab1, ws.wts);
    MI355_LAUNCH_CHECK();
    AggPoolArgs a{};
    a.fm = fm; a.B = B; a.C = C; a.HW = HW; a.W = W; a.R = 1;
    a.plan = agg_plan(C, HW, 1);
    a.wts = ws.wts; a.vals = ws.vals; a.q = ws.q;
    AggRegions rg{};
    rg.packed[0] = (unsigned)H << 16 | (unsigned)W << 24;
    agg_pool(AG_CROW, st, a, rg);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_crow_finish, dim3((unsigned)B), dim3(AG_THREADS), 0, st, (const float*)ws.vals, (const float*)ws.q, C,
                       normalize ? 1 : 0, eps, out);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
