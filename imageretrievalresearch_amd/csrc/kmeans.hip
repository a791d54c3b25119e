// Spherical k-means beside the nearest-centroid pass (rank_common.h: NearestEpi; driver nearest_centroid in rank.hip): the
// members of every cluster as CSR (mi355_cluster_members), the centroid update (mi355_centroid_update[_f16]) and the
// contingency table of two labelings (mi355_contingency).  Every result is the same bits on every run and every device:
// counts are integers, and every floating-point sum is taken in float64 in an order fixed by the data alone.  gfx950 only.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

typedef _Float16 f16;

// The update's summation order: the members of a cluster in ascending row index, KM_SEG at a time into one float64 partial
// sum per (segment, column), then the partial sums in segment order.  Both constants are part of the result's bits; neither
// depends on the device (whiten.hip's MO_WGS is the precedent).
constexpr int KM_SEG = 256;        // members per partial sum
constexpr int KM_COLS = 256;       // columns per workgroup: a member row is read as one 1 KB (fp16: 512 B) piece

__device__ __forceinline__ i64 block_sum_i64(i64 v, i64* sh) {      // 256 threads; every thread gets the sum
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// counts[k] = the rows assigned to k: one workgroup per cluster scans the assignment vector.  Workgroup 0 also checks the
// range of every value (flag[0] = 1 on a value outside [0, K): an argument error the host reports).
__global__ __launch_bounds__(256) void k_member_counts(const i64* __restrict__ assign, i64 N, i64 K, i64* __restrict__ counts,
                                                       unsigned* __restrict__ flag) {
    __shared__ i64 sh[4];
    const i64 k = blockIdx.x;
    i64 c = 0;
    bool bad = false;
    for (i64 i = threadIdx.x; i < N; i += 256) {
        const i64 a = assign[i];
        c += a == k;
        bad = bad || a < 0 || a >= K;
    }
    if (k == 0 && bad) flag[0] = 1u;
    c = block_sum_i64(c, sh);
    if (threadIdx.x == 0) counts[k] = c;
}

// offsets[0 .. K] = the exclusive scan of counts, segoff[0 .. K] that of the clusters' segment counts cdiv(counts, KM_SEG):
// one workgroup, each thread a contiguous run of clusters (k_range_scan's scheme)
__global__ __launch_bounds__(1024) void k_member_offsets(const i64* __restrict__ counts, i64 K, i64* __restrict__ offsets,
                                                         i64* __restrict__ segoff) {
    __shared__ i64 pc[1024], ps[1024];
    const int tid = threadIdx.x;
    const i64 per = (K + 1023) / 1024, b0 = tid * per < K ? tid * per : K, b1 = b0 + per < K ? b0 + per : K;
    i64 c = 0, s = 0;
    for (i64 i = b0; i < b1; ++i) {
        c += counts[i];
        s += (counts[i] + KM_SEG - 1) / KM_SEG;
    }
    pc[tid] = c;
    ps[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const i64 vc = tid >= d ? pc[tid - d] : 0, vs = tid >= d ? ps[tid - d] : 0;
        __syncthreads();
        pc[tid] += vc;
        ps[tid] += vs;
        __syncthreads();
    }
    c = pc[tid] - c;
    s = ps[tid] - s;
    if (tid == 0) { offsets[0] = 0; if (segoff) segoff[0] = 0; }
    for (i64 i = b0; i < b1; ++i) {
        c += counts[i];
        s += (counts[i] + KM_SEG - 1) / KM_SEG;
        offsets[i + 1] = c;
        if (segoff) segoff[i + 1] = s;
    }
}

// order[offsets[k] ..) = the rows assigned to k, ascending: one workgroup per cluster scans the assignment vector 256 rows at
// a time and compacts its matches with a ballot per wave and a prefix over the four waves.  The writes stay inside the
// cluster's slice because k_member_counts counted the same vector.
__global__ __launch_bounds__(256) void k_member_order(const i64* __restrict__ assign, i64 N, const i64* __restrict__ offsets,
                                                      i64* __restrict__ order) {
    __shared__ int wcnt[4];
    const i64 k = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 base = offsets[k];
    const i64 end = offsets[k + 1];
    for (i64 i0 = 0; i0 < N && base < end; i0 += 256) {
        const i64 i = i0 + threadIdx.x;
        const bool m = i < N && assign[i] == k;
        const unsigned long long b = __ballot(m);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int before = __popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) before += wcnt[w];
        const int total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (m && base + before < end) order[base + before] = i;
        base += total;
        __syncthreads();
    }
}

__device__ __forceinline__ double widen(float v) { return (double)v; }
__device__ __forceinline__ double widen(f16 v) { return (double)(float)v; }      // exact

// partial[s][col] = the float64 sum of column col over the members of segment s, in ascending row order.  Workgroup
// (s, column chunk): segment s belongs to the cluster k with segoff[k] <= s < segoff[k + 1] (binary search).
template <class T>
__global__ __launch_bounds__(256) void k_centroid_partial(const T* __restrict__ rows, i64 ld, int D, i64 K,
                                                          const i64* __restrict__ offsets, const i64* __restrict__ segoff,
                                                          const i64* __restrict__ order, double* __restrict__ partial) {
    const i64 s = blockIdx.x;
    if (s >= segoff[K]) return;
    i64 lo = 0, hi = K - 1;                       // the last k with segoff[k] <= s (empty clusters share a value: skip them)
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (segoff[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const i64 k = lo;
    const i64 m0 = offsets[k] + (s - segoff[k]) * KM_SEG;
    const i64 m1 = m0 + KM_SEG < offsets[k + 1] ? m0 + KM_SEG : offsets[k + 1];
    const int col = blockIdx.y * KM_COLS + threadIdx.x;
    if (col >= D) return;
    double sum = 0.0;
    i64 m = m0;
    for (; m + 4 <= m1; m += 4) {                 // four loads in flight, added in member order
        const T v0 = rows[order[m] * ld + col], v1 = rows[order[m + 1] * ld + col];
        const T v2 = rows[order[m + 2] * ld + col], v3 = rows[order[m + 3] * ld + col];
        sum += widen(v0);
        sum += widen(v1);
        sum += widen(v2);
        sum += widen(v3);
    }
    for (; m < m1; ++m) sum += widen(rows[order[m] * ld + col]);
    partial[s * D + col] = sum;
}

// One workgroup per cluster: the partial sums in segment order, |sum| over the columns (each thread its columns ascending,
// then a fixed tree), c = sum / max(|sum|, eps) in float64 rounded once to fp32.  No member, or |sum| < eps: the previous row.
// previous and centroids may be one buffer (each element is read, then written, by one thread), so neither is __restrict__.
__global__ __launch_bounds__(256) void k_centroid_finish(double* __restrict__ partial, int D, const i64* __restrict__ offsets,
                                                         const i64* __restrict__ segoff, const float* previous, double eps,
                                                         float* centroids, i64* __restrict__ counts) {
    __shared__ double sh[4];
    const i64 k = blockIdx.x;
    const i64 s0 = segoff[k], ns = segoff[k + 1] - s0, cnt = offsets[k + 1] - offsets[k];
    double* tot = partial + s0 * D;               // (ns > 0) the cluster's sums replace its first segment's
    double ss = 0.0;
    if (ns > 0)
        for (int col = threadIdx.x; col < D; col += 256) {
            double s = 0.0;
            for (i64 j = 0; j < ns; ++j) s += partial[(s0 + j) * D + col];
            tot[col] = s;
            ss += s * s;
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) ss += __shfl_xor(ss, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ss;
    __syncthreads();
    const double norm = sqrt(((sh[0] + sh[1]) + sh[2]) + sh[3]);
    const bool keep = cnt == 0 || norm < eps;
    for (int col = threadIdx.x; col < D; col += 256)
        centroids[k * D + col] = keep ? previous[k * D + col] : (float)(tot[col] / norm);
    if (threadIdx.x == 0) counts[k] = cnt;
}

// ---- contingency table of two labelings a[N] in [0, Ka), b[N] in [0, Kb)
constexpr int CT_LDS_CELLS = 8192;                 // Ka * Kb up to this: a u32 sub-histogram per workgroup in LDS (32 KB)
constexpr int CT_WGS = 1024;                       // workgroups at most

template <bool LDS>
__global__ __launch_bounds__(256) void k_contingency(const i64* __restrict__ a, const i64* __restrict__ b, i64 N, i64 Ka, i64 Kb,
                                                     unsigned long long* __restrict__ table, unsigned* __restrict__ flag) {
    extern __shared__ unsigned bins[];
    const int cells = (int)(Ka * Kb);
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < cells; i += 256) bins[i] = 0u;
        __syncthreads();
    }
    bool bad = false;
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
        const i64 x = a[i], y = b[i];
        if (x < 0 || x >= Ka || y < 0 || y >= Kb) { bad = true; continue; }
        if constexpr (LDS) atomicAdd(&bins[x * Kb + y], 1u);
        else atomicAdd(&table[x * Kb + y], 1ull);
    }
    if (bad) flag[0] = 1u;
    if constexpr (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += 256)
            if (bins[i]) atomicAdd(&table[i], (unsigned long long)bins[i]);
    }
}

// ---- host side
struct KmeansWs {
    unsigned* flag; i64* counts; i64* segoff; double* partial; size_t total;
};
static i64 max_segments(i64 N, i64 K) { return (N + KM_SEG - 1) / KM_SEG + K; }
// One workgroup of 256 threads per cluster (members) or per segment (update): a grid dimension holds fewer than 2^32
// threads, so at most 2^24 - 1 workgroups.
constexpr i64 KM_MAX_WGS = ((i64)1 << 24) - 1;
// flag word, counts [K], segoff [K + 1], and (dim > 0) the partial sums [max_segments][dim]
static KmeansWs kmeans_carve(void* ws, i64 N, i64 K, int dim) {
    KmeansWs r{};
    WsCarver c(ws);
    r.flag = (unsigned*)c.take(sizeof(unsigned));
    r.counts = (i64*)c.take((size_t)K * sizeof(i64));
    r.segoff = (i64*)c.take((size_t)(K + 1) * sizeof(i64));
    r.partial = (double*)c.take(dim > 0 ? (size_t)max_segments(N, K) * dim * sizeof(double) : 0);
    r.total = c.total();
    return r;
}

static int check_members(const int64_t* assign, i64 N, i64 K, const int64_t* offsets, const int64_t* order, const char* who) {
    MI355_REQUIRE(assign && offsets && order, "%s: null assign/offsets/order pointer", who);
    MI355_REQUIRE(N >= 1, "%s: N=%lld must be >= 1", who, (long long)N);
    MI355_REQUIRE(K >= 1 && K <= KM_MAX_WGS, "%s: n_clusters=%lld outside [1, 2^24)", who, (long long)K);
    return OK;
}

// offsets, order (and w.counts, w.segoff) from assign; reads the range flag back (one host sync)
static int members(const int64_t* assign, i64 N, i64 K, int64_t* offsets, int64_t* order, const KmeansWs& w, hipStream_t st,
                   const char* who) {
    RoctxRange range("kmeans/members");
    MI355_CHECK_HIP(hipMemsetAsync(w.flag, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_member_counts, dim3((unsigned)K), dim3(256), 0, st, (const i64*)assign, N, K, w.counts, w.flag);
    MI355_LAUNCH_CHECK();
    unsigned bad = 0;
    MI355_CHECK_HIP(hipMemcpyAsync(&bad, w.flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    MI355_REQUIRE(!bad, "%s: assign holds a value outside [0, n_clusters=%lld)", who, (long long)K);
    hipLaunchKernelGGL(k_member_offsets, dim3(1), dim3(1024), 0, st, (const i64*)w.counts, K, (i64*)offsets, w.segoff);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_member_order, dim3((unsigned)K), dim3(256), 0, st, (const i64*)assign, N, (const i64*)offsets, (i64*)order);
    MI355_LAUNCH_CHECK();
    return OK;
}

// mi355_cluster_members for a caller inside the library that must not wait for the host (the IVF scan, ivf.hip): the same
// three kernels, and the range flag stays on the device (*flag, zeroed here, 1 after a value outside [0, K)) for the caller
// to read with its own.  A value out of range belongs to no cluster: it is counted nowhere and appears nowhere in order.
size_t members_ws_bytes(i64 N, i64 K) { return kmeans_carve(nullptr, N, K, 0).total; }
int members_async(const int64_t* assign, i64 N, i64 K, int64_t* offsets, int64_t* order, void* workspace, hipStream_t st,
                  const unsigned** flag) {
    const KmeansWs w = kmeans_carve(workspace, N, K, 0);
    RoctxRange range("kmeans/members");
    MI355_CHECK_HIP(hipMemsetAsync(w.flag, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_member_counts, dim3((unsigned)K), dim3(256), 0, st, (const i64*)assign, N, K, w.counts, w.flag);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_member_offsets, dim3(1), dim3(1024), 0, st, (const i64*)w.counts, K, (i64*)offsets, w.segoff);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_member_order, dim3((unsigned)K), dim3(256), 0, st, (const i64*)assign, N, (const i64*)offsets, (i64*)order);
    MI355_LAUNCH_CHECK();
    *flag = w.flag;
    return OK;
}

static int centroid_update(const void* rows, bool f16rows, i64 ld, i64 N, int dim, const int64_t* assign, i64 K, const float* previous,
                           float eps, float* centroids, int64_t* counts, int64_t* offsets, int64_t* order, void* workspace,
                           size_t workspace_bytes, void* stream, const char* who) {
    MI355_REQUIRE(rows && previous && centroids && counts, "%s: null rows/previous/centroids/counts pointer", who);
    if (int e = check_members(assign, N, K, offsets, order, who)) return e;
    MI355_REQUIRE(dim >= 1, "%s: dim=%d must be >= 1", who, dim);
    MI355_REQUIRE(!f16rows || ((uintptr_t)rows & 15) == 0, "%s: fp16 rows must be 16-byte aligned", who);
    MI355_REQUIRE(N <= KM_MAX_WGS * KM_SEG && max_segments(N, K) <= KM_MAX_WGS,
                  "%s: shape too large N=%lld n_clusters=%lld: more than 2^24 - 1 segments of %d rows", who, (long long)N,
                  (long long)K, KM_SEG);
    const KmeansWs w = kmeans_carve(workspace, N, K, dim);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    if (int e = members(assign, N, K, offsets, order, w, st, who)) return e;
    RoctxRange range("kmeans/update");
    const dim3 grid((unsigned)max_segments(N, K), (unsigned)cdiv(dim, KM_COLS));
    if (f16rows)
        hipLaunchKernelGGL((k_centroid_partial<f16>), grid, dim3(256), 0, st, (const f16*)rows, ld, dim, K, (const i64*)offsets,
                           (const i64*)w.segoff, (const i64*)order, w.partial);
    else
        hipLaunchKernelGGL((k_centroid_partial<float>), grid, dim3(256), 0, st, (const float*)rows, ld, dim, K, (const i64*)offsets,
                           (const i64*)w.segoff, (const i64*)order, w.partial);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_centroid_finish, dim3((unsigned)K), dim3(256), 0, st, w.partial, dim, (const i64*)offsets,
                       (const i64*)w.segoff, previous, (double)eps, centroids, (i64*)counts);
    MI355_LAUNCH_CHECK();
    return OK;
}

static int f16_row_ld(int dim) { return (dim + 63) / 64 * 64; }      // the row length of mi355_gallery_to_f16

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_cluster_members_workspace_bytes(int64_t N, int64_t K) {
    if (N < 1 || K < 1) return 0;
    return kmeans_carve(nullptr, N, K, 0).total;
}

int mi355_cluster_members(const int64_t* assign, int64_t N, int64_t K, int64_t* offsets, int64_t* order, void* workspace,
                          size_t workspace_bytes, void* stream) {
    const char* who = "cluster_members";
    if (int e = check_members(assign, N, K, offsets, order, who)) return e;
    const KmeansWs w = kmeans_carve(workspace, N, K, 0);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    return members(assign, N, K, offsets, order, w, (hipStream_t)stream, who);
}

size_t mi355_centroid_update_workspace_bytes(int64_t N, int64_t K, int dim) {
    if (N < 1 || K < 1 || dim < 1) return 0;
    return kmeans_carve(nullptr, N, K, dim).total;
}

size_t mi355_centroid_update_f16_workspace_bytes(int64_t N, int64_t K, int dim) {
    return mi355_centroid_update_workspace_bytes(N, K, dim);      // the partial sums are float64 for either kind of rows
}

int mi355_centroid_update(const float* rows, int64_t N, int dim, const int64_t* assign, int64_t K, const float* previous, float eps,
                          float* centroids, int64_t* counts, int64_t* offsets, int64_t* order, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return centroid_update(rows, false, dim, N, dim, assign, K, previous, eps, centroids, counts, offsets, order, workspace,
                           workspace_bytes, stream, "centroid_update");
}

int mi355_centroid_update_f16(const void* rows_f16, int64_t N, int dim, const int64_t* assign, int64_t K, const float* previous,
                              float eps, float* centroids, int64_t* counts, int64_t* offsets, int64_t* order, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return centroid_update(rows_f16, true, dim >= 1 ? f16_row_ld(dim) : 0, N, dim, assign, K, previous, eps, centroids, counts,
                           offsets, order, workspace, workspace_bytes, stream, "centroid_update_f16");
}

size_t mi355_contingency_workspace_bytes(int64_t N, int64_t Ka, int64_t Kb) {
    if (N < 1 || Ka < 1 || Kb < 1) return 0;
    return 512;                                    // the flag word, with room to align it
}

int mi355_contingency(const int64_t* a, const int64_t* b, int64_t N, int64_t Ka, int64_t Kb, int64_t* table, void* workspace,
                      size_t workspace_bytes, void* stream) {
    const char* who = "contingency";
    MI355_REQUIRE(a && b && table, "%s: null a/b/table pointer", who);
    MI355_REQUIRE(N >= 1 && N <= ((int64_t)1 << 40), "%s: N=%lld outside [1, 2^40]", who, (long long)N);
    MI355_REQUIRE(Ka >= 1 && Kb >= 1, "%s: Ka=%lld Kb=%lld must be >= 1", who, (long long)Ka, (long long)Kb);
    MI355_REQUIRE(Ka <= ((int64_t)1 << 28) && Kb <= ((int64_t)1 << 28) && Ka * Kb <= ((int64_t)1 << 28),
                  "%s: table too large: Ka * Kb = %lld * %lld > 2^28 cells", who, (long long)Ka, (long long)Kb);
    const size_t need = mi355_contingency_workspace_bytes(N, Ka, Kb);
    MI355_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    unsigned* flag = (unsigned*)align256(workspace);
    RoctxRange range("kmeans/contingency");
    MI355_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), st));
    MI355_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)(Ka * Kb) * sizeof(int64_t), st));
    const unsigned wgs = (unsigned)(cdiv(N, 256 * 16) < CT_WGS ? cdiv(N, 256 * 16) : CT_WGS);
    if (Ka * Kb <= CT_LDS_CELLS)
        hipLaunchKernelGGL((k_contingency<true>), dim3(wgs), dim3(256), (size_t)(Ka * Kb) * sizeof(unsigned), st, (const i64*)a,
                           (const i64*)b, (i64)N, (i64)Ka, (i64)Kb, (unsigned long long*)table, flag);
    else
        hipLaunchKernelGGL((k_contingency<false>), dim3(wgs), dim3(256), 0, st, (const i64*)a, (const i64*)b, (i64)N, (i64)Ka,
                           (i64)Kb, (unsigned long long*)table, flag);
    MI355_LAUNCH_CHECK();
    unsigned bad = 0;
    MI355_CHECK_HIP(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    MI355_REQUIRE(!bad, "%s: a label outside [0, Ka=%lld) x [0, Kb=%lld)", who, (long long)Ka, (long long)Kb);
    return OK;
}

}  // extern "C"
