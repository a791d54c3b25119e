// k-reciprocal re-ranking (Zhong, Zheng, Cao and Li, CVPR 2017), gallery-graph variant: mi355_kr_sets, mi355_kr_weights,
// mi355_kr_local_qe, mi355_kr_score (include/mi355_retrieval.h has the definitions).  gfx950 only.
//
// The kNN lists come from the library's own search; everything here is integer set work on <= 32-entry lists, one gather-dot
// and sparse merges, all on CSR rows (offsets int64, cols int32 ascending, vals fp32).  No kernel has an atomic and every
// floating-point sum is taken in an order that depends only on the row it belongs to, so a result never depends on how the
// rows were batched.
//
//   k_kr_sets      one wave (a 64-thread workgroup) per row: R(r) by ballots over the row's list, the expansion by a loop over
//                  the candidates of R(r) (R_h(c) in lanes 0 .. h), the set kept unsorted in LDS (<= 561 entries) and written
//                  in ascending order by rank counting.  Count pass -> k_kr_scan -> fill pass.
//   k_kr_weights   one workgroup per row, the row's own vector once in LDS as fp32; one wave per (row, column) dot: 16-byte
//                  loads of the gallery row, lane-strided fp32 sums, a shuffle reduction; exp(s - 1), then the row's sum by
//                  one wave in lane-strided order and the division.
//   k_kr_local_qe  one wave per row: lane s walks source row s (<= 33 sorted sparse rows), a wave minimum picks the next
//                  column, the values of the sources that hold it are added in source order.  Count pass, scan, fill pass.
//   k_kr_score     one workgroup per query with V'(q) in LDS; a wave per shortlist row looks each of its columns up in V'(q)
//                  by binary search and sums the minima lane-strided, then a shuffle reduction.
// Every index read from a list or a CSR row is range-checked before it addresses memory.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <math.h>

namespace mi355 {

typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int KR_MAX_K1 = MI355_KR_MAX_K1;
constexpr int KR_MAX_ROW = (KR_MAX_K1 + 1) * ((KR_MAX_K1 + 1) / 2 + 1);   // 33 * 17 = 561: |R| <= 33, <= 16 new per candidate
constexpr int KR_SET_LD = 576;
static_assert(KR_MAX_ROW <= KR_SET_LD, "the set of a row fits its LDS buffer");
constexpr int KR_SCORE_LDS = 4096;      // entries of V'(q) the score kernel keeps in LDS (longer rows are read where they lie)
constexpr int KR_MAX_DIM = 8192;        // the row's own vector in LDS: 32 KB

// The CSR row r as [lo, lo + n): empty when the offsets are not a row inside [0, nnz)
__device__ __forceinline__ int csr_row(const i64* __restrict__ offsets, i64 r, i64 nnz, i64& lo) {
    lo = offsets[r];
    const i64 hi = offsets[r + 1];
    if (lo < 0 || hi < lo || hi > nnz || hi - lo > INT_MAX) return 0;
    return (int)(hi - lo);
}

// Whether a lane t' < t of the first n lanes holds the same (valid) row j: lists of a search never repeat a row, a list given
// by hand may
__device__ __forceinline__ bool seen_before(int j, int t, int n) {
    bool dup = false;
    for (int s = 0; s < n; ++s) {
        const int js = __shfl(j, s, 64);
        dup |= s < t && js == j;
    }
    return dup;
}

__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) {
    return __popcll(mask & ((1ull << lane) - 1ull));
}

struct SetArgs {
    const i64* lists;       // [R][k1] neighbour rows of each row
    const float* lvals;     // [R][k1] their scores (query rows), or null (gallery rows: row r IS gallery row r)
    const float* tau;       // [G] k1-th neighbour score of each gallery row (query rows)
    const i64* graph;       // [G][k1] neighbour rows of each gallery row
    i64 R, G;
    int k1;
    i64* offsets;           // [R + 1]
    int* cols;              // fill pass: [cap]; null: count pass
    i64 cap;
};

__global__ __launch_bounds__(64) void k_kr_sets(SetArgs a) {
    __shared__ int S[KR_SET_LD];
    const int lane = threadIdx.x, k1 = a.k1, h = (k1 + 1) / 2;
    const i64 row = blockIdx.x;
    const bool query = a.lvals != nullptr;
    // 1. R(row): lane t holds neighbour t
    int j = -1;
    bool mem = false;
    if (lane < k1) {
        const i64 jj = a.lists[row * k1 + lane];
        if (jj >= 0 && jj < a.G && (query || jj != row)) j = (int)jj;
    }
    if (j >= 0) {
        if (query) {
            mem = a.lvals[row * k1 + lane] >= a.tau[j];
        } else {
            const i64* nj = a.graph + (i64)j * k1;
            for (int s = 0; s < k1; ++s) mem |= nj[s] == row;
        }
    }
    const bool dup = seen_before(j, lane, k1);             // every lane takes part in the shuffles
    mem = mem && !dup;
    const unsigned long long rb = __ballot(mem);
    const int own = query ? 0 : 1;
    if (!query && lane == 0) S[0] = (int)row;
    if (mem) S[own + lanes_below(rb, lane)] = j;
    const int nR = own + __popcll(rb);
    int n = nR;
    __syncthreads();
    // 2. the expansion: every candidate c of the unexpanded R, R_h(c) = {c} + reciprocal neighbours among the first h
    for (int ci = 0; ci < nR; ++ci) {
        const int c = S[ci];
        int m = -1;
        bool in = false;
        if (lane < h) {
            const i64 mm = a.graph[(i64)c * k1 + lane];
            if (mm >= 0 && mm < a.G && mm != c) m = (int)mm;
            if (m >= 0) {
                const i64* nm = a.graph + (i64)m * k1;
                for (int s = 0; s < h; ++s) in |= nm[s] == c;
            }
        }
        const bool again = seen_before(m, lane, h);
        in = in && !again;
        if (lane == h) { m = c; in = true; }
        const int size = __popcll(__ballot(in));
        bool inR = false, inE = false;
        if (in) {
            for (int p = 0; p < nR; ++p) inR |= S[p] == m;
            for (int p = nR; p < n; ++p) inE |= S[p] == m;
        }
        const int common = __popcll(__ballot(inR));
        const bool fresh = in && !inR && !inE && 3 * common > 2 * size;
        const unsigned long long fb = __ballot(fresh);
        const int add = __popcll(fb);
        __syncthreads();                                   // every lane has read S before it grows
        if (fresh && n + add <= KR_SET_LD) S[n + lanes_below(fb, lane)] = m;
        if (n + add <= KR_SET_LD) n += add;
        __syncthreads();
    }
    // 3. count, or the set in ascending order (rank counting: the entries are distinct)
    if (!a.cols) {
        if (lane == 0) a.offsets[row + 1] = n;
        return;
    }
    const i64 off = a.offsets[row];
    if (off < 0 || off + n > a.cap || a.offsets[row + 1] - off != n) return;
    for (int i = lane; i < n; i += 64) {
        const int x = S[i];
        int rank = 0;
        for (int p = 0; p < n; ++p) rank += S[p] < x;
        a.cols[off + rank] = x;
    }
}

// offsets[0] = 0, offsets[r + 1] = counts of rows 0 .. r (the counts lie in offsets[1 ..] on entry): one workgroup, a
// contiguous chunk of rows per thread
__global__ __launch_bounds__(1024) void k_kr_scan(i64* offsets, i64 R) {
    __shared__ i64 part[1024];
    const int tid = threadIdx.x;
    const i64 chunk = (R + 1023) / 1024, r0 = (i64)tid * chunk, r1 = r0 + chunk < R ? r0 + chunk : R;
    i64 s = 0;
    for (i64 r = r0; r < r1; ++r) s += offsets[r + 1];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const i64 v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    i64 run = part[tid] - s;
    if (tid == 0) offsets[0] = 0;
    for (i64 r = r0; r < r1; ++r) {
        run += offsets[r + 1];
        offsets[r + 1] = run;
    }
}

struct WeightArgs {
    const void* rows; int rows_f16; i64 rows_ld; i64 R;
    const void* gal; i64 G; i64 gld; int dim;
    const i64* offsets; const int* cols; i64 nnz;
    float* vals;
};

// W elements of a gallery row at unit u, times the same elements of the staged row
template <int W>
__device__ __forceinline__ float dot_unit(const float* g, const float* xs, int u, float acc) {
    if constexpr (W == 4) {
        const f32x4 v = reinterpret_cast<const f32x4*>(g)[u], x = reinterpret_cast<const f32x4*>(xs)[u];
        acc = fmaf(v.x, x.x, acc); acc = fmaf(v.y, x.y, acc); acc = fmaf(v.z, x.z, acc); acc = fmaf(v.w, x.w, acc);
        return acc;
    } else {
        return fmaf(g[u], xs[u], acc);
    }
}
template <int W>
__device__ __forceinline__ float dot_unit(const f16* g, const float* xs, int u, float acc) {
    if constexpr (W == 8) {
        const f16x8 v = reinterpret_cast<const f16x8*>(g)[u];
        const f32x4 x0 = reinterpret_cast<const f32x4*>(xs)[2 * u], x1 = reinterpret_cast<const f32x4*>(xs)[2 * u + 1];
        acc = fmaf((float)v[0], x0.x, acc); acc = fmaf((float)v[1], x0.y, acc);
        acc = fmaf((float)v[2], x0.z, acc); acc = fmaf((float)v[3], x0.w, acc);
        acc = fmaf((float)v[4], x1.x, acc); acc = fmaf((float)v[5], x1.y, acc);
        acc = fmaf((float)v[6], x1.z, acc); acc = fmaf((float)v[7], x1.w, acc);
        return acc;
    } else {
        return fmaf((float)g[u], xs[u], acc);
    }
}

template <class TG, int W>
__global__ __launch_bounds__(256) void k_kr_weights(WeightArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];    // [dim] the row's own vector, then [1] the row's sum
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, dim = a.dim;
    const i64 row = blockIdx.x;
    i64 lo;
    const int n = csr_row(a.offsets, row, a.nnz, lo);
    if (n == 0) return;
    if (a.rows_f16) {
        const f16* x = static_cast<const f16*>(a.rows) + row * a.rows_ld;
        for (int i = tid; i < dim; i += 256) xs[i] = (float)x[i];
    } else {
        const float* x = static_cast<const float*>(a.rows) + row * a.rows_ld;
        for (int i = tid; i < dim; i += 256) xs[i] = x[i];
    }
    __syncthreads();
    const TG* gal = static_cast<const TG*>(a.gal);
    const int nu = dim / W;
    float* out = a.vals + lo;
    for (int c = wave; c < n; c += 4) {
        const int j = a.cols[lo + c];
        const bool ok = j >= 0 && j < a.G;                 // wave-uniform
        float acc = 0.f;
        if (ok) {
            const TG* g = gal + (i64)j * a.gld;
            for (int u = lane; u < nu; u += 64) acc = dot_unit<W>(g, xs, u, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) out[c] = ok ? expf(acc - 1.0f) : 0.f;     // exp(-d), d = 1 - s
    }
    __syncthreads();                                       // the workgroup's own stores are visible to it
    if (wave == 0) {
        float s = 0.f;
        for (int i = lane; i < n; i += 64) s += out[i];
        s = wave_sum(s);
        if (lane == 0) xs[dim] = s;
    }
    __syncthreads();
    const float tot = xs[dim];
    for (int i = tid; i < n; i += 256) out[i] = out[i] / tot;
}

struct LocalArgs {
    const i64* lists; i64 R; int k1, k2;
    const i64* own_off; const int* own_cols; const float* own_vals; i64 own_nnz;
    const i64* g_off; const int* g_cols; const float* g_vals; i64 G, g_nnz;
    i64* out_off; int* out_cols; float* out_vals; i64 cap;
};

__global__ __launch_bounds__(64) void k_kr_local_qe(LocalArgs a) {
    const int lane = threadIdx.x;
    const i64 row = blockIdx.x;
    // lane s < k2 walks source s: the row itself, then its first k2 - 1 neighbours' gallery rows
    const int* cols = nullptr;
    const float* vals = nullptr;
    int len = 0;
    if (lane == 0) {
        i64 lo;
        len = csr_row(a.own_off, row, a.own_nnz, lo);
        cols = a.own_cols + lo;
        vals = a.own_vals + lo;
    } else if (lane < a.k2) {
        const i64 j = a.lists[row * a.k1 + lane - 1];
        if (j >= 0 && j < a.G) {
            i64 lo;
            len = csr_row(a.g_off, j, a.g_nnz, lo);
            cols = a.g_cols + lo;
            vals = a.g_vals + lo;
        }
    }
    const bool fill = a.out_cols != nullptr;
    const i64 off = fill ? a.out_off[row] : 0, end = fill ? a.out_off[row + 1] : 0;
    const bool fits = off >= 0 && end <= a.cap;            // a row that does not fit is not written, as in k_kr_sets
    const float k2f = (float)a.k2;
    int cur = 0, n = 0;
    int head = cur < len ? cols[cur] : INT_MAX;
    float hv = cur < len && fill ? vals[cur] : 0.f;
    for (;;) {
        int m = head;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
        if (m == INT_MAX) break;
        const bool mine = head == m;
        if (fill) {
            const float c = mine ? hv : 0.f;
            float sum = 0.f;
            for (int s = 0; s < a.k2; ++s) sum += __shfl(c, s, 64);      // source order; an absent source adds 0
            if (lane == 0 && fits && off + n < end) {
                a.out_cols[off + n] = m;
                a.out_vals[off + n] = sum / k2f;
            }
        }
        ++n;
        if (mine) {
            ++cur;
            head = cur < len ? cols[cur] : INT_MAX;
            hv = cur < len && fill ? vals[cur] : 0.f;
        }
    }
    if (!fill && lane == 0) a.out_off[row + 1] = n;
}

struct ScoreArgs {
    const i64* q_off; const int* q_cols; const float* q_vals; i64 q_nnz; i64 Q;
    const i64* g_off; const int* g_cols; const float* g_vals; i64 g_nnz; i64 G;
    const float* svals; const i64* sidx; int K;
    float lam;
    float* out;
};

__global__ __launch_bounds__(256) void k_kr_score(ScoreArgs a) {
    __shared__ int qc[KR_SCORE_LDS];
    __shared__ float qv[KR_SCORE_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 q = blockIdx.x;
    i64 qlo;
    const int nq = csr_row(a.q_off, q, a.q_nnz, qlo);
    const int* pc = a.q_cols + qlo;
    const float* pv = a.q_vals + qlo;
    if (nq <= KR_SCORE_LDS) {                              // block-uniform
        for (int i = tid; i < nq; i += 256) { qc[i] = pc[i]; qv[i] = pv[i]; }
        pc = qc;
        pv = qv;
        __syncthreads();
    }
    for (int p = wave; p < a.K; p += 4) {
        const i64 g = a.sidx[q * a.K + p];
        if (g < 0 || g >= a.G) {                           // a pad of the shortlist stays a pad
            if (lane == 0) a.out[q * a.K + p] = NEG_INF;
            continue;
        }
        i64 glo;
        const int ng = csr_row(a.g_off, g, a.g_nnz, glo);
        float part = 0.f;
        for (int i = lane; i < ng; i += 64) {
            const int c = a.g_cols[glo + i];
            int lo = 0, hi = nq;                           // first position with pc[pos] >= c
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pc[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < nq && pc[lo] == c) part += fminf(a.g_vals[glo + i], pv[lo]);
        }
        const float m = wave_sum(part);
        if (lane == 0) {
            const float dj = 1.0f - m / (2.0f - m);
            const float s = a.svals[q * a.K + p];
            a.out[q * a.K + p] = 1.0f - ((1.0f - a.lam) * dj + a.lam * (1.0f - s));
        }
    }
}

static bool kr_aligned(const void* p, i64 ld, int elem) { return ((uintptr_t)p & 15) == 0 && (ld * elem) % 16 == 0; }

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_kr_sets(const int64_t* lists, const float* list_vals, const float* tau, int64_t R, int k1, const int64_t* graph,
                  int64_t G, int64_t* offsets, int32_t* cols, int64_t cols_capacity, void* stream) {
    const char* who = "kr_sets";
    MI355_REQUIRE(lists && graph && offsets, "%s: null pointer", who);
    MI355_REQUIRE(k1 >= 1 && k1 <= KR_MAX_K1, "%s: k1=%d outside [1, %d]", who, k1, KR_MAX_K1);
    MI355_REQUIRE(R >= 0 && G >= 1 && R <= INT_MAX && G <= INT_MAX, "%s: bad shape R=%lld G=%lld", who, (long long)R, (long long)G);
    MI355_REQUIRE((list_vals != nullptr) == (tau != nullptr), "%s: query rows need both list_vals and tau, gallery rows neither",
                  who);
    MI355_REQUIRE(list_vals || R == G, "%s: gallery rows are the whole graph (R=%lld, G=%lld)", who, (long long)R, (long long)G);
    MI355_REQUIRE(!cols || cols_capacity >= 0, "%s: cols_capacity=%lld < 0", who, (long long)cols_capacity);
    if (R == 0) return OK;
    hipStream_t st = (hipStream_t)stream;
    SetArgs a{(const i64*)lists, list_vals, tau, (const i64*)graph, R, G, k1, (i64*)offsets, cols, cols_capacity};
    hipLaunchKernelGGL(k_kr_sets, dim3((unsigned)R), dim3(64), 0, st, a);
    MI355_LAUNCH_CHECK();
    if (!cols) {
        hipLaunchKernelGGL(k_kr_scan, dim3(1), dim3(1024), 0, st, (i64*)offsets, (i64)R);
        MI355_LAUNCH_CHECK();
    }
    return OK;
}

int mi355_kr_weights(const void* rows, int rows_dtype, int64_t rows_ld, int64_t R, const void* gallery, int gallery_dtype,
                     int64_t G, int64_t gallery_ld, int dim, const int64_t* offsets, const int32_t* cols, int64_t nnz,
                     float* vals, void* stream) {
    const char* who = "kr_weights";
    MI355_REQUIRE(rows && gallery && offsets, "%s: null pointer", who);
    MI355_REQUIRE(nnz >= 0 && (nnz == 0 || (cols && vals)), "%s: nnz=%lld needs cols and vals", who, (long long)nnz);
    for (int d : {rows_dtype, gallery_dtype})
        MI355_REQUIRE(d == MI355_DTYPE_F32 || d == MI355_DTYPE_F16, "%s: dtype %d is neither MI355_DTYPE_F32 nor MI355_DTYPE_F16",
                      who, d);
    MI355_REQUIRE(dim >= 1 && dim <= KR_MAX_DIM, "%s: dim=%d outside [1, %d]", who, dim, KR_MAX_DIM);
    MI355_REQUIRE(R >= 0 && G >= 1 && R <= INT_MAX && G <= INT_MAX, "%s: bad shape R=%lld G=%lld", who, (long long)R, (long long)G);
    MI355_REQUIRE(rows_ld >= dim && gallery_ld >= dim, "%s: leading dims must be >= dim=%d (rows_ld=%lld gallery_ld=%lld)", who,
                  dim, (long long)rows_ld, (long long)gallery_ld);
    if (R == 0 || nnz == 0) return OK;
    WeightArgs a{rows, rows_dtype == MI355_DTYPE_F16, rows_ld, R, gallery, G, gallery_ld, dim, (const i64*)offsets, cols, nnz, vals};
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)dim + 4) * sizeof(float);
    const dim3 grid((unsigned)R), block(256);
    if (gallery_dtype == MI355_DTYPE_F16) {
        if (dim % 8 == 0 && kr_aligned(gallery, gallery_ld, 2)) hipLaunchKernelGGL((k_kr_weights<f16, 8>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((k_kr_weights<f16, 1>), grid, block, lds, st, a);
    } else {
        if (dim % 4 == 0 && kr_aligned(gallery, gallery_ld, 4)) hipLaunchKernelGGL((k_kr_weights<float, 4>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((k_kr_weights<float, 1>), grid, block, lds, st, a);
    }
    MI355_LAUNCH_CHECK();
    return OK;
}

int mi355_kr_local_qe(const int64_t* lists, int64_t R, int k1, int k2, const int64_t* own_offsets, const int32_t* own_cols,
                      const float* own_vals, int64_t own_nnz, const int64_t* gallery_offsets, const int32_t* gallery_cols,
                      const float* gallery_vals, int64_t gallery_nnz, int64_t G, int64_t* out_offsets, int32_t* out_cols,
                      float* out_vals, int64_t out_capacity, void* stream) {
    const char* who = "kr_local_qe";
    MI355_REQUIRE(lists && own_offsets && gallery_offsets && out_offsets, "%s: null pointer", who);
    MI355_REQUIRE(k1 >= 1 && k1 <= KR_MAX_K1, "%s: k1=%d outside [1, %d]", who, k1, KR_MAX_K1);
    MI355_REQUIRE(k2 >= 1 && k2 <= k1 + 1, "%s: k2=%d outside [1, k1 + 1 = %d]", who, k2, k1 + 1);
    MI355_REQUIRE(R >= 0 && G >= 1 && R <= INT_MAX && G <= INT_MAX, "%s: bad shape R=%lld G=%lld", who, (long long)R, (long long)G);
    MI355_REQUIRE(own_nnz >= 0 && (own_nnz == 0 || (own_cols && own_vals)), "%s: own_nnz=%lld needs cols and vals", who,
                  (long long)own_nnz);
    MI355_REQUIRE(gallery_nnz >= 0 && (gallery_nnz == 0 || (gallery_cols && gallery_vals)), "%s: gallery_nnz=%lld needs cols and vals",
                  who, (long long)gallery_nnz);
    MI355_REQUIRE((out_cols != nullptr) == (out_vals != nullptr), "%s: the fill pass needs both out_cols and out_vals", who);
    MI355_REQUIRE(!out_cols || out_capacity >= 0, "%s: out_capacity=%lld < 0", who, (long long)out_capacity);
    if (R == 0) return OK;
    hipStream_t st = (hipStream_t)stream;
    LocalArgs a{(const i64*)lists, R, k1, k2, (const i64*)own_offsets, own_cols, own_vals, own_nnz, (const i64*)gallery_offsets,
                gallery_cols, gallery_vals, G, gallery_nnz, (i64*)out_offsets, out_cols, out_vals, out_capacity};
    hipLaunchKernelGGL(k_kr_local_qe, dim3((unsigned)R), dim3(64), 0, st, a);
    MI355_LAUNCH_CHECK();
    if (!out_cols) {
        hipLaunchKernelGGL(k_kr_scan, dim3(1), dim3(1024), 0, st, (i64*)out_offsets, (i64)R);
        MI355_LAUNCH_CHECK();
    }
    return OK;
}

int mi355_kr_score(const int64_t* query_offsets, const int32_t* query_cols, const float* query_vals, int64_t query_nnz, int64_t Q,
                   const int64_t* gallery_offsets, const int32_t* gallery_cols, const float* gallery_vals, int64_t gallery_nnz,
                   int64_t G, const float* shortlist_vals, const int64_t* shortlist_idx, int K, float lam, float* out,
                   void* stream) {
    const char* who = "kr_score";
    MI355_REQUIRE(query_offsets && gallery_offsets && shortlist_vals && shortlist_idx && out, "%s: null pointer", who);
    MI355_REQUIRE(Q >= 0 && G >= 1 && Q <= INT_MAX && G <= INT_MAX, "%s: bad shape Q=%lld G=%lld", who, (long long)Q, (long long)G);
    MI355_REQUIRE(K >= 1 && K <= LARGE_K, "%s: shortlist K=%d outside [1, %d]", who, K, LARGE_K);
    MI355_REQUIRE(isfinite(lam) && lam >= 0.f && lam <= 1.f, "%s: lam must be in [0, 1], got %g", who, (double)lam);
    MI355_REQUIRE(query_nnz >= 0 && (query_nnz == 0 || (query_cols && query_vals)), "%s: query_nnz=%lld needs cols and vals", who,
                  (long long)query_nnz);
    MI355_REQUIRE(gallery_nnz >= 0 && (gallery_nnz == 0 || (gallery_cols && gallery_vals)), "%s: gallery_nnz=%lld needs cols and vals",
                  who, (long long)gallery_nnz);
    if (Q == 0) return OK;
    ScoreArgs a{(const i64*)query_offsets, query_cols, query_vals, query_nnz, Q, (const i64*)gallery_offsets, gallery_cols,
                gallery_vals, gallery_nnz, G, shortlist_vals, (const i64*)shortlist_idx, K, lam, out};
    hipLaunchKernelGGL(k_kr_score, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, a);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
