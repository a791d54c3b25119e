// Diffusion re-ranking (Iscen et al., CVPR 2017; truncated as in Yang et al., AAAI 2019): conjugate gradients on the part of a
// gallery's kNN graph that a query's shortlist induces.  include/mi355_retrieval.h states every step.
//   mi355_diffusion_graph ... the symmetric normalised affinity rows (cols / vals / deg) of a kNN graph, two launches: one
//                             thread per row finds the mutual edges, takes the smaller of the two affinities and sums the row's
//                             degree in slot order; one thread per slot then scales by 1 / sqrt(d_i d_j).
//   mi355_diffusion_source .. y = max(score, 0)^gamma on the first kq shortlist slots.
//   mi355_diffusion_solve ... one workgroup per query.  In LDS: a row -> position table of the shortlist (open addressing, at
//                             least twice as many slots as rows, so it cannot fill), the local position of every slot of every
//                             shortlist row (uint16, slot-major so that a wave reads consecutive halfwords) and the search
//                             direction p.  f, r and A p of a row are only ever touched by the thread that owns the row and
//                             stay in its registers (DF_ROWS rows per thread); the values S(i, t) are re-read from the index.
// Every dot product is summed per thread in row order, per wave by xor shuffles and across the waves in wave order: a query's
// bits depend on its own inputs alone.  Every loop is bounded before it starts; no workgroup waits on another; no global
// atomics.  gfx950 only.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef long long i64;

constexpr int DF_THREADS = 256, DF_WAVES = DF_THREADS / 64;
constexpr int DF_MAX_L = 1024, DF_MAX_KD = MI355_DIFFUSION_MAX_KD, DF_MAX_ITERS = 64, DF_MAX_GAMMA = 8;
constexpr int DF_ROWS = DF_MAX_L / DF_THREADS;         // shortlist rows a thread owns: tid, tid + 256, ...
constexpr unsigned DF_EMPTY = 0xffffffffu;             // a free key of the table (rows are below 2^31)
constexpr unsigned short DF_NONE = 0xffffu;            // a slot without a local edge
constexpr float DF_FREEZE = 3.5527136788005009e-15f;   // 2^-48

// x^gamma by repeated multiplication, left to right
__device__ __forceinline__ float df_pow(float x, int gamma) {
    float a = x;
    for (int g = 1; g < gamma; ++g) a *= x;
    return a;
}

// ---- the index
struct DfGraphArgs {
    const i64* nn;      // [G][kd]
    const float* nv;    // [G][kd]
    i64 G;
    int kd, gamma;
    int* cols;          // [G][kd]
    float* vals;        // [G][kd]: w after the first launch, S after the second
    float* deg;         // [G]
};

__global__ __launch_bounds__(DF_THREADS) void k_df_edges(DfGraphArgs a) {
    const i64 i = (i64)blockIdx.x * DF_THREADS + threadIdx.x;
    if (i >= a.G) return;
    float d = 0.f;
    for (int t = 0; t < a.kd; ++t) {
        const i64 j = a.nn[i * a.kd + t];
        int col = -1;
        float w = 0.f;
        if (j >= 0 && j < a.G) {
            const i64* lj = a.nn + j * a.kd;
            int u = -1;
            for (int s = a.kd - 1; s >= 0; --s) u = lj[s] == i ? s : u;     // the first slot of i in j's list
            if (u >= 0) {
                col = (int)j;
                w = fminf(df_pow(fmaxf(a.nv[i * a.kd + t], 0.f), a.gamma), df_pow(fmaxf(a.nv[j * a.kd + u], 0.f), a.gamma));
            }
        }
        a.cols[i * a.kd + t] = col;
        a.vals[i * a.kd + t] = w;
        d += w;
    }
    a.deg[i] = d;
}

__device__ __forceinline__ float df_rsqrt_deg(float d) { return d > 0.f ? 1.f / sqrtf(d) : 0.f; }

__global__ __launch_bounds__(DF_THREADS) void k_df_normalise(DfGraphArgs a) {
    const i64 e = (i64)blockIdx.x * DF_THREADS + threadIdx.x;
    if (e >= a.G * a.kd) return;
    const int j = a.cols[e];
    if (j < 0) return;                                                      // empty: the 0 of the first launch stays
    a.vals[e] = a.vals[e] * (df_rsqrt_deg(a.deg[e / a.kd]) * df_rsqrt_deg(a.deg[j]));
}

// ---- the source vector
__global__ __launch_bounds__(DF_THREADS) void k_df_source(const float* sv, const i64* si, i64 n, int L, int kq, int gamma, float* y) {
    const i64 e = (i64)blockIdx.x * DF_THREADS + threadIdx.x;
    if (e >= n) return;
    y[e] = ((int)(e % L) < kq && si[e] >= 0) ? df_pow(fmaxf(sv[e], 0.f), gamma) : 0.f;
}

// ---- the solve
struct DfSolveArgs {
    const int* cols;      // [G][kd]
    const float* vals;    // [G][kd]
    i64 G;
    int kd, L, iters;
    unsigned tsize;       // slots of the row -> position table, a power of two >= 2 L
    const i64* si;        // [Q][L] local rows, outside [0, G): a pad
    const float* y;       // [Q][L]
    float alpha;
    float* f;             // [Q][L]
    int* out_iters;       // [Q] or null
};

// The dynamic LDS of one workgroup, in this order
struct DfLds {
    size_t keys, tpos, p, red, pos, total;
};
static inline unsigned df_table_slots(int L) {
    unsigned t = 8;
    while (t < 2u * (unsigned)L) t <<= 1;
    return t;
}
static inline DfLds df_lds(int L, int kd) {
    DfLds l{};
    size_t o = 0;
    const unsigned tsize = df_table_slots(L);
    l.keys = o; o += (size_t)tsize * sizeof(unsigned);                     // the table's rows
    l.tpos = o; o += (size_t)tsize * sizeof(unsigned);                     // and their (earliest) shortlist position
    l.p = o; o += (size_t)L * sizeof(float);                               // the search direction
    l.red = o; o += 2 * DF_WAVES * sizeof(float);                          // the waves' partial sums, two buffers
    l.pos = o; o += align_up((size_t)L * kd * sizeof(unsigned short), 16); // [kd][L] local positions
    l.total = o;
    return l;
}
static bool df_solve_shape_ok(int L, int kd) { return L >= 1 && L <= DF_MAX_L && kd >= 1 && kd <= DF_MAX_KD; }

// The sum of v over the workgroup, the same bits in every thread.  `red` alternates between two buffers, so one barrier per sum
// is enough: a buffer is written again only two sums later, behind the barrier of the sum in between.
__device__ __forceinline__ float df_block_sum(float v, float* red, int& flip) {
    v = wave_sum(v);
    float* buf = red + flip * DF_WAVES;
    flip ^= 1;
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = buf[0];
#pragma unroll
    for (int w = 1; w < DF_WAVES; ++w) s += buf[w];
    return s;
}

__global__ __launch_bounds__(DF_THREADS) void k_df_solve(DfSolveArgs a, DfLds lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* keys = reinterpret_cast<unsigned*>(smem + lds.keys);
    unsigned* tpos = reinterpret_cast<unsigned*>(smem + lds.tpos);
    float* p = reinterpret_cast<float*>(smem + lds.p);
    float* red = reinterpret_cast<float*>(smem + lds.red);
    unsigned short* pos = reinterpret_cast<unsigned short*>(smem + lds.pos);
    const int tid = threadIdx.x, L = a.L, kd = a.kd;
    const i64 q = blockIdx.x;
    const i64* si = a.si + q * L;
    const unsigned tmask = a.tsize - 1u;
    const int tshift = 32 - (31 - __builtin_clz(a.tsize));                  // the top log2(tsize) bits of the hash

    for (unsigned i = tid; i < a.tsize; i += DF_THREADS) {
        keys[i] = DF_EMPTY;
        tpos[i] = DF_EMPTY;
    }
    __syncthreads();
    // the table: every real row of the shortlist, with the earliest position that holds it
    for (int r = tid; r < L; r += DF_THREADS) {
        const i64 g = si[r];
        if (g < 0 || g >= a.G) continue;
        const unsigned key = (unsigned)g;
        unsigned h = (key * 2654435761u) >> tshift;
        for (unsigned t = 0; t < a.tsize; ++t) {
            const unsigned old = atomicCAS(&keys[h], DF_EMPTY, key);
            if (old == DF_EMPTY || old == key) {
                atomicMin(&tpos[h], (unsigned)r);
                break;
            }
            h = (h + 1u) & tmask;
        }
    }
    __syncthreads();
    // the local position of every slot: pos[t][r], DF_NONE where the edge is empty or leaves the shortlist
    for (int e = tid; e < L * kd; e += DF_THREADS) {
        const int r = e / kd, t = e - r * kd;
        const i64 g = si[r];
        unsigned short ps = DF_NONE;
        if (g >= 0 && g < a.G) {
            const int c = a.cols[g * kd + t];
            if (c >= 0) {
                const unsigned key = (unsigned)c;
                unsigned h = (key * 2654435761u) >> tshift;
                for (unsigned s = 0; s < a.tsize; ++s) {
                    const unsigned k = keys[h];
                    if (k == key) ps = (unsigned short)tpos[h];
                    if (k == key || k == DF_EMPTY) break;
                    h = (h + 1u) & tmask;
                }
            }
        }
        pos[t * L + r] = ps;
    }

    // f0 = 0, r0 = p0 = y
    float fv[DF_ROWS], rv[DF_ROWS], ap[DF_ROWS];
    i64 base[DF_ROWS];                                                      // where the row's values start; -1: a pad
    int flip = 0;
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < DF_ROWS; ++j) {
        const int r = tid + j * DF_THREADS;
        fv[j] = 0.f; rv[j] = 0.f; ap[j] = 0.f; base[j] = -1;
        if (r < L) {
            const i64 g = si[r];
            if (g >= 0 && g < a.G) {
                base[j] = g * kd;
                rv[j] = a.y[q * L + r];
            }
            p[r] = rv[j];
            part += rv[j] * rv[j];
        }
    }
    float rs = df_block_sum(part, red, flip);                               // its barrier also publishes pos and p
    const float stop = DF_FREEZE * rs;
    int done = 0;
    for (int it = 0; it < a.iters; ++it) {
        if (rs <= stop) break;                                              // converged, or y = 0
        // A p = p - alpha S p on the thread's own rows, S p summed in slot order
        part = 0.f;
#pragma unroll
        for (int j = 0; j < DF_ROWS; ++j) {
            const int r = tid + j * DF_THREADS;
            if (r < L) {
                float sp = 0.f;
                if (base[j] >= 0) {
                    const float* v = a.vals + base[j];
                    for (int t = 0; t < kd; ++t) {
                        const unsigned short ps = pos[t * L + r];
                        if (ps != DF_NONE) sp += v[t] * p[ps];
                    }
                }
                const float pr = p[r];
                ap[j] = pr - a.alpha * sp;
                part += pr * ap[j];
            }
        }
        const float pap = df_block_sum(part, red, flip);
        if (!(pap > 0.f)) break;                                            // the same in every thread
        const float step = rs / pap;
        part = 0.f;
#pragma unroll
        for (int j = 0; j < DF_ROWS; ++j) {
            const int r = tid + j * DF_THREADS;
            if (r < L) {
                fv[j] += step * p[r];
                rv[j] -= step * ap[j];
                part += rv[j] * rv[j];
            }
        }
        const float rs_new = df_block_sum(part, red, flip);                 // behind its barrier nobody reads the old p
        const float beta = rs_new / rs;
#pragma unroll
        for (int j = 0; j < DF_ROWS; ++j) {
            const int r = tid + j * DF_THREADS;
            if (r < L) p[r] = rv[j] + beta * p[r];
        }
        rs = rs_new;
        ++done;
        __syncthreads();                                                    // the new p is whole
    }
#pragma unroll
    for (int j = 0; j < DF_ROWS; ++j) {
        const int r = tid + j * DF_THREADS;
        if (r < L) a.f[q * L + r] = base[j] >= 0 ? fv[j] : -INFINITY;
    }
    if (tid == 0 && a.out_iters) a.out_iters[q] = done;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_diffusion_graph(const int64_t* nn, const float* nv, int64_t G, int kd, int gamma, int32_t* cols, float* vals, float* deg,
                          void* stream) {
    const char* who = "diffusion_graph";
    MI355_REQUIRE(nn && nv && cols && vals && deg, "%s: null nn/nv/cols/vals/deg pointer", who);
    MI355_REQUIRE(kd >= 1 && kd <= DF_MAX_KD, "%s: kd=%d outside [1, %d]", who, kd, DF_MAX_KD);
    MI355_REQUIRE(G > kd && G <= INT_MAX, "%s: G=%lld must be above kd=%d and below 2^31", who, (long long)G, kd);
    MI355_REQUIRE(gamma >= 1 && gamma <= DF_MAX_GAMMA, "%s: gamma=%d outside [1, %d]", who, gamma, DF_MAX_GAMMA);
    RoctxRange range("diffusion/graph");
    hipStream_t st = (hipStream_t)stream;
    const DfGraphArgs a{(const i64*)nn, nv, G, kd, gamma, cols, vals, deg};
    hipLaunchKernelGGL(k_df_edges, dim3((unsigned)cdiv(G, DF_THREADS)), dim3(DF_THREADS), 0, st, a);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_df_normalise, dim3((unsigned)cdiv(G * kd, DF_THREADS)), dim3(DF_THREADS), 0, st, a);
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_diffusion_source(const float* shortlist_vals, const int64_t* shortlist_idx, int64_t Q, int L, int kq, int gamma, float* y,
                           void* stream) {
    const char* who = "diffusion_source";
    MI355_REQUIRE(shortlist_vals && shortlist_idx && y, "%s: null shortlist/y pointer", who);
    MI355_REQUIRE(Q >= 0 && Q <= INT_MAX, "%s: Q=%lld outside [0, 2^31)", who, (long long)Q);
    MI355_REQUIRE(L >= 1 && L <= DF_MAX_L, "%s: shortlist L=%d outside [1, %d]", who, L, DF_MAX_L);
    MI355_REQUIRE(kq >= 1 && kq <= L, "%s: kq=%d outside [1, L=%d]", who, kq, L);
    MI355_REQUIRE(gamma >= 1 && gamma <= DF_MAX_GAMMA, "%s: gamma=%d outside [1, %d]", who, gamma, DF_MAX_GAMMA);
    if (Q == 0) return OK;
    RoctxRange range("diffusion/source");
    hipLaunchKernelGGL(k_df_source, dim3((unsigned)cdiv(Q * L, DF_THREADS)), dim3(DF_THREADS), 0, (hipStream_t)stream, shortlist_vals,
                       (const i64*)shortlist_idx, (i64)Q * L, L, kq, gamma, y);
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t mi355_diffusion_lds_bytes(int L, int kd) { return df_solve_shape_ok(L, kd) ? df_lds(L, kd).total : 0; }

int mi355_diffusion_solve(const int32_t* cols, const float* vals, int64_t G, int kd, const int64_t* shortlist_idx, const float* y,
                          int64_t Q, int L, float alpha, int iters, float* f, int32_t* iterations, void* stream) {
    const char* who = "diffusion_solve";
    MI355_REQUIRE(cols && vals && shortlist_idx && y && f, "%s: null cols/vals/shortlist/y/f pointer", who);
    MI355_REQUIRE(kd >= 1 && kd <= DF_MAX_KD, "%s: kd=%d outside [1, %d]", who, kd, DF_MAX_KD);
    MI355_REQUIRE(G >= 1 && G <= INT_MAX, "%s: G=%lld outside [1, 2^31)", who, (long long)G);
    MI355_REQUIRE(Q >= 0 && Q <= INT_MAX, "%s: Q=%lld outside [0, 2^31)", who, (long long)Q);
    MI355_REQUIRE(L >= 1 && L <= DF_MAX_L, "%s: shortlist L=%d outside [1, %d]", who, L, DF_MAX_L);
    MI355_REQUIRE(iters >= 1 && iters <= DF_MAX_ITERS, "%s: iters=%d outside [1, %d]", who, iters, DF_MAX_ITERS);
    MI355_REQUIRE(isfinite(alpha) && alpha > 0.f && alpha < 1.f, "%s: alpha must be a finite float in (0, 1), got %g", who,
                  (double)alpha);
    const DfLds lds = df_lds(L, kd);
    MI355_REQUIRE(df_solve_shape_ok(L, kd) && lds.total <= 160u * 1024u, "%s: %zu bytes of LDS for L=%d kd=%d", who, lds.total, L, kd);
    if (Q == 0) return OK;
    RoctxRange range("diffusion/solve");
    // up to 84 KB of dynamic LDS: raise the kernel's limit once per device (as graph.hip and pq.hip do)
    static bool raised[MI355_MAX_DEVICES] = {false};
    if (first_time_on_this_device(raised))
        MI355_CHECK_HIP(hipFuncSetAttribute((const void*)k_df_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)df_lds(DF_MAX_L, DF_MAX_KD).total));
    const DfSolveArgs a{cols, vals, G, kd, L, iters, df_table_slots(L), (const i64*)shortlist_idx, y, alpha, f, iterations};
    hipLaunchKernelGGL(k_df_solve, dim3((unsigned)Q), dim3(DF_THREADS), lds.total, (hipStream_t)stream, a, lds);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
