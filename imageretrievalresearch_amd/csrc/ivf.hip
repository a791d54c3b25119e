// Inverted-file (IVF) search: the scan of the lists a query probes (mi355_ivf_scan).  The gallery's rows are read where they
// lie, through the lists' CSR (offsets, order); the candidates of every query go to a slab that mi355_merge_topk selects
// from.  Nothing is read back to the host between the steps:
//   1. the queries are normalised (mi355_l2_normalize_rows);
//   2. the (query, list) pairs are grouped by list: the kernels of mi355_cluster_members over the flattened probes;
//   3. k_ivf_bases: per query the running sum of its probed lists' lengths = the slot base of each pair, and n_q;
//   4. k_ivf_plan / k_ivf_items: the work items (list, group of up to NQ pairs, chunk of IVF_CHUNK rows) and their count;
//   5. k_ivf_pad: the slots n_q .. cap - 1 of every query;
//   6. k_ivf_scan: a fixed grid loops over the items; one wave per row, the group's queries in LDS.
// Every slot is written by exactly one wave (of k_ivf_scan below n_q, of k_ivf_pad from n_q on).
// mi355_ivf_scan_i8 is the same pipeline over an int8 gallery's codes: step 1 makes the queries' two int8 planes and s_q
// instead (k_ivf_queries_i8, the normalisation folded in), and the scan's rows are scored by integer dot products (Int8Rows
// below); steps 2 - 5 and the loop over the items are shared.  gfx950 only.
#include "i8_quant.h"
#include "ivf_lists.h"
#include "row_dot.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

constexpr int IVF_NQ = 4;                  // queries of one group at most (k_cos_gemv's count)
constexpr int IVF_NQ_I8 = 8;               // over int8 rows: a query is 2 bytes per element in LDS, not 4
constexpr int IVF_CHUNK = 64;              // rows of one work item: 16 per wave
constexpr size_t IVF_LDS = 64 * 1024;      // the group's queries

// What the kernels share
struct IvfArgs {
    const float* qn;        // [Q][dim] normalised queries (fp32 / fp16 rows)
    const i32x4* planes;    // [Q][hi, lo][ldq] the queries' int8 planes (int8 rows)
    const float* sq;        // [Q] s_q (int8 rows)
    const float* scales;    // [G] s_g (int8 rows)
    const void* rows;       // fp32 / fp16 rows, or int8 codes
    i64 ld, G;              // ld: elements between rows
    const i64* offsets;     // [nlist + 1]
    const i64* order;       // [G]
    i64 nlist;
    const i64* probes;      // [Q][nprobe]
    i64 Q;
    int nprobe, dim, ldq, nq;      // ldq: floats of one query in LDS (dim rounded up to a unit; int8 rows: the bytes of one
                                   // plane, dim rounded up to 128); nq: queries of a group
    i64 cap, idx_offset;
    const i64* poff;        // [nlist + 1]: the pairs of list l are pord[poff[l] .. poff[l + 1])
    const i64* pord;        // [Q * nprobe] pair ids q * nprobe + j, ascending within a list
    i64* base;              // [Q * nprobe] the slot base of a pair
    i64* nfill;             // [Q] n_q
    i64* wstart;            // [nlist + 1] the first work item of a list
    int4* items;            // [max_work] (list, group, chunk)
    i64 max_work;
    i64* n_work;
    float* cand_val;
    i64* cand_idx;
    unsigned* flag;         // [IVF_FLAGS]
    RankFilter filt;
    bool filtered;
};

// base[q][j] = the rows of probes[q][0 .. j); nfill[q] = n_q.  One thread per query.
__global__ __launch_bounds__(256) void k_ivf_bases(IvfArgs a) {
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.Q) return;
    i64 run = 0;
    bool bad = false;
    for (int j = 0; j < a.nprobe; ++j) {
        const i64 l = a.probes[q * a.nprobe + j];
        i64 b = 0, e = 0;
        if (l < 0 || l >= a.nlist) bad = true;                      // in no list's pairs either: never scanned
        else if (!list_range(a.offsets, l, a.G, b, e)) bad = true;
        a.base[q * a.nprobe + j] = run;
        run += e - b;
    }
    a.nfill[q] = run;
    if (bad) a.flag[IVF_FLAG_ENTRY] = 1u;
    if (run > a.cap) a.flag[IVF_FLAG_CAP] = 1u;
}

// wstart[0 .. nlist] = the exclusive scan of the lists' item counts cdiv(pairs, nq) * cdiv(rows, IVF_CHUNK), n_work = their
// sum (at most max_work): one workgroup, each thread a contiguous run of lists (k_member_offsets' scheme)
__device__ __forceinline__ i64 list_items(const IvfArgs& a, i64 l) {
    i64 b, e;
    list_range(a.offsets, l, a.G, b, e);
    const i64 pairs = a.poff[l + 1] - a.poff[l];
    return ((pairs + a.nq - 1) / a.nq) * ((e - b + IVF_CHUNK - 1) / IVF_CHUNK);
}
__global__ __launch_bounds__(1024) void k_ivf_plan(IvfArgs a) {
    __shared__ i64 pc[1024];
    const int tid = threadIdx.x;
    const i64 K = a.nlist;
    const i64 per = (K + 1023) / 1024, b0 = tid * per < K ? tid * per : K, b1 = b0 + per < K ? b0 + per : K;
    i64 c = 0;
    for (i64 l = b0; l < b1; ++l) c += list_items(a, l);
    pc[tid] = c;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const i64 v = tid >= d ? pc[tid - d] : 0;
        __syncthreads();
        pc[tid] += v;
        __syncthreads();
    }
    c = pc[tid] - c;
    if (tid == 0) a.wstart[0] = 0;
    for (i64 l = b0; l < b1; ++l) {
        c += list_items(a, l);
        a.wstart[l + 1] = c;
    }
    if (tid == 1023) {
        // more than max_work items: some n_q passes cap (k_ivf_bases flags it); the scan stops at what the table holds
        a.n_work[0] = c < a.max_work ? c : a.max_work;
    }
}

// items[wstart[l] ..) = (l, group, chunk), the chunks of one group next to each other.  One workgroup per list.
__global__ __launch_bounds__(256) void k_ivf_items(IvfArgs a) {
    const i64 l = blockIdx.x;
    i64 b, e;
    list_range(a.offsets, l, a.G, b, e);
    const i64 nch = (e - b + IVF_CHUNK - 1) / IVF_CHUNK;
    const i64 w0 = a.wstart[l], cnt = a.wstart[l + 1] - w0;
    for (i64 i = threadIdx.x; i < cnt; i += 256) {
        if (w0 + i >= a.max_work) break;
        a.items[w0 + i] = make_int4((int)l, (int)(i / nch), (int)(i % nch), 0);
    }
}

// The slots n_q .. cap - 1 of every query: "no candidate"
__global__ __launch_bounds__(256) void k_ivf_pad(IvfArgs a) {
    const i64 n = a.Q * a.cap, stride = (i64)gridDim.x * 256;
    for (i64 t = (i64)blockIdx.x * 256 + threadIdx.x; t < n; t += stride) {
        const i64 q = t / a.cap, s = t - q * a.cap;
        if (s >= a.nfill[q]) {
            a.cand_val[t] = NEG_INF;
            a.cand_idx[t] = NO_CAND_IDX;
        }
    }
}

// How the scan scores the rows of one kind of gallery.  A policy P has MAXQ (queries of a group at most), load_group (the
// group's n queries into LDS, by the whole workgroup), Lane / lane_state (what lane i < NQ keeps of its own query) and
// score<NQ> (one wave: row g against the group's queries; lane i < NQ returns the score of query i).  With AHEAD a wave reads
// the ids of its rows in one load before it scores the first.
template <bool F16, bool VEC>
struct FloatRows {
    static constexpr int MAXQ = IVF_NQ;
    static constexpr bool AHEAD = false;
    struct Lane {};
    static __device__ __forceinline__ Lane lane_state(const IvfArgs&, i64, bool) { return {}; }
    static __device__ __forceinline__ void load_group(const IvfArgs& a, float* smem, i64 p0, int n) {   // [nq][ldq]
        for (int i = threadIdx.x; i < n * a.ldq; i += 256) {
            const int qi = i / a.ldq, e = i - qi * a.ldq;
            const i64 q = a.pord[p0 + qi] / a.nprobe;
            smem[i] = e < a.dim ? a.qn[q * a.dim + e] : 0.f;
        }
    }
    template <int NQ>
    static __device__ __forceinline__ float score(const IvfArgs& a, const float* smem, i64 g, int lane, const Lane&) {
        float acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
        row_dot<NQ, F16, VEC>(a, g, smem, lane, acc);
        float mine = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float t = wave_sum(acc[q]);
            if (lane == q) mine = t;
        }
        return mine;
    }
};

// int8 codes (rank_i8.hip's k_cos_gemv_i8 per row): 16 bytes of the row per lane and load, up to four loads in flight, the
// group's planes in LDS as [nq][hi, lo][ldq] bytes, sdot4 into int32, an integer wave reduction, then the float tail of every
// int8 score.  The sums are exact, so the bits are those of mi355_rank_topk_i8 for the pair.
struct Int8Rows {
    static constexpr int MAXQ = IVF_NQ_I8;
    static constexpr bool AHEAD = true;
    struct Lane { float sq; };
    static __device__ __forceinline__ Lane lane_state(const IvfArgs& a, i64 myq, bool mine) { return {mine ? a.sq[myq] : 0.f}; }
    static __device__ __forceinline__ void load_group(const IvfArgs& a, float* smem, i64 p0, int n) {
        i32x4* qs = reinterpret_cast<i32x4*>(smem);
        const int per = a.ldq / 8;                                  // 16-byte chunks of one query: two planes
        for (int i = threadIdx.x; i < n * per; i += 256) {
            const int qi = i / per, e = i - qi * per;
            const i64 q = a.pord[p0 + qi] / a.nprobe;
            qs[i] = a.planes[q * per + e];
        }
    }
    template <int NQ>
    static __device__ __forceinline__ float score(const IvfArgs& a, const float* smem, i64 g, int lane, const Lane& st) {
        const i32x4* qs = reinterpret_cast<const i32x4*>(smem);
        const int nch = a.ldq / 16;                                 // 16-byte chunks of a row (its padding is zero)
        const i32x4* row = reinterpret_cast<const i32x4*>((const signed char*)a.rows + g * a.ld);
        int hi[NQ], lo[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { hi[q] = 0; lo[q] = 0; }
        for (int c0 = 0; c0 < nch; c0 += 4 * 64) {
            i32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                v[u] = c < nch ? row[c] : (i32x4){0, 0, 0, 0};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 64 + lane;
                if (c < nch) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const i32x4 h = qs[(q * 2) * nch + c], l = qs[(q * 2 + 1) * nch + c];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            hi[q] = __builtin_amdgcn_sdot4(h[e], v[u][e], hi[q], false);
                            lo[q] = __builtin_amdgcn_sdot4(l[e], v[u][e], lo[q], false);
                        }
                    }
                }
            }
        }
        int mh = 0, ml = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            int h = hi[q], l = lo[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { h += __shfl_xor(h, o, 64); l += __shfl_xor(l, o, 64); }
            if (lane == q) { mh = h; ml = l; }
        }
        return i8_score(mh, ml, st.sq, a.scales[g]);
    }
};

// The rows [r0, r1) of list l (whose rows begin at order[lb]) against the NQ pairs pord[p0 ..): wave w takes rows r0 + w,
// r0 + w + 4, ...; lane i < NQ writes the slot of pair i.  With P::AHEAD lane i reads the id of the wave's i-th row in one
// load up front: an int8 row is short, and the chain order -> row -> score of one row after the other bounds the plain loop.
template <class P, int NQ>
__device__ __forceinline__ void scan_chunk(const IvfArgs& a, const float* __restrict__ qs, i64 p0, i64 lb, i64 r0, i64 r1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 myq = 0, mybase = 0, lab = 0, ex = -1;
    if (lane < NQ) {
        const i64 pair = a.pord[p0 + lane];
        myq = pair / a.nprobe;
        mybase = a.base[pair];
        if (a.filtered) query_filter(a.filt, myq, lab, ex);
    }
    const typename P::Lane st = P::lane_state(a, myq, lane < NQ);
    auto put = [&](i64 r, i64 g, bool ok, float mine) {
        if (lane < NQ) {
            const i64 slot = mybase + (r - lb);
            if (slot < a.cap) {                                     // n_q > cap: flagged by k_ivf_bases
                bool el = ok;
                if (ok && a.filtered) {
                    const i64 gl = a.filt.mode != MI355_LABEL_ANY ? a.filt.glab[g] : 0;
                    el = eligible(a.filt.mode, lab, gl, ex, g);
                }
                a.cand_val[myq * a.cap + slot] = el ? mine : NEG_INF;
                a.cand_idx[myq * a.cap + slot] = el ? g + a.idx_offset : NO_CAND_IDX;
            }
        }
    };
    if constexpr (!P::AHEAD) {
        for (i64 r = r0 + wave; r < r1; r += 4) {
            const i64 g = a.order[r];
            const bool ok = g >= 0 && g < a.G;                      // the same for the whole wave
            float mine = 0.f;
            if (ok) mine = P::template score<NQ>(a, qs, g, lane, st);
            else if (lane == 0) a.flag[IVF_FLAG_ENTRY] = 1u;
            put(r, g, ok, mine);
        }
    } else {
        const int nrows = r0 + wave < r1 ? (int)((r1 - r0 - wave + 3) / 4) : 0;     // at most IVF_CHUNK / 4
        const i64 mine_r = r0 + wave + 4 * (i64)lane;
        const long long gl = lane < nrows ? a.order[mine_r] : -1;   // lane i: the id of the wave's i-th row
#pragma unroll 1                                                    // one row at a time: 89 VGPRs, five waves per SIMD
        for (int i = 0; i < nrows; ++i) {
            const i64 g = (i64)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(gl >> 32), i) << 32) |
                                (unsigned)__builtin_amdgcn_readlane((int)gl, i));     // in scalar registers, as a load of it
            const bool ok = g >= 0 && g < a.G;
            float mine = 0.f;
            if (ok) mine = P::template score<NQ>(a, qs, g, lane, st);
            else if (lane == 0) a.flag[IVF_FLAG_ENTRY] = 1u;
            put(r0 + wave + 4 * (i64)i, g, ok, mine);
        }
    }
}

template <class P>
__global__ __launch_bounds__(256) void k_ivf_scan(IvfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float qs[];     // the group's queries, as P lays them out
    const i64 nw = a.n_work[0];
    for (i64 w = blockIdx.x; w < nw; w += gridDim.x) {
        const int4 it = a.items[w];
        const i64 l = it.x;
        i64 lb, le;
        list_range(a.offsets, l, a.G, lb, le);
        const i64 p0 = a.poff[l] + (i64)it.y * a.nq;
        const i64 left = a.poff[l + 1] - p0;
        const int n = (int)(left < a.nq ? left : a.nq);
        const i64 r0 = lb + (i64)it.z * IVF_CHUNK, r1 = r0 + IVF_CHUNK < le ? r0 + IVF_CHUNK : le;
        __syncthreads();                                            // the previous item's reads of qs are done
        P::load_group(a, qs, p0, n);
        __syncthreads();
#define IVF_CASE(N) case N: if constexpr (N <= P::MAXQ) scan_chunk<P, N>(a, qs, p0, lb, r0, r1); break;
        switch (n) {                                                // the same for the whole workgroup
            IVF_CASE(1) IVF_CASE(2) IVF_CASE(3) IVF_CASE(4) IVF_CASE(5) IVF_CASE(6) IVF_CASE(7) IVF_CASE(8)
            default: break;
        }
#undef IVF_CASE
    }
}

// The queries of a scan over int8 rows: raw fp32 rows -> the two int8 planes [Q][hi, lo][lq] and s_q [Q], one wave per query.
// n = the fp32 row mi355_l2_normalize_rows writes (row_inv_norm, i8_norm_elem: k_rows_to_i8's way), then the split of
// k_split_queries_i8 element by element; the bytes dim .. lq - 1 are zero.
__global__ __launch_bounds__(256) void k_ivf_queries_i8(const float* __restrict__ in, signed char* __restrict__ planes,
                                                        float* __restrict__ sq, i64 Q, int dim, int lq, float eps, int vec) {
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Q) return;
    const float* x = in + row * dim;
    const float r = row_inv_norm(x, dim, eps, vec, lane);
    float amax = 0.f;
    bool nan = false;
    for (int i = lane; i < dim; i += 64) {
        const float n = i8_norm_elem(x[i], r);
        nan = nan || n != n;
        amax = fmaxf(amax, fabsf(n));
    }
    const I8Quant q = i8_quant(wave_max(amax), __ballot(nan) != 0ull);
    if (lane == 0) sq[row] = q.scale;
    const float lo_mul = i8_lo_mul(q);
    unsigned* hi = reinterpret_cast<unsigned*>(planes + row * 2 * lq);
    unsigned* lo = hi + lq / 4;
    for (int w = lane; w < lq / 4; w += 64) {
        int h[4] = {0, 0, 0, 0}, l[4] = {0, 0, 0, 0};
        if (!q.zero) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (w * 4 + e < dim) i8_split_elem(i8_norm_elem(x[w * 4 + e], r), q, lo_mul, h[e], l[e]);
        }
        hi[w] = pack4_i8(h[0], h[1], h[2], h[3]);
        lo[w] = pack4_i8(l[0], l[1], l[2], l[3]);
    }
}

// ---- host side
static int ivf_ldq(int dim, bool f16rows) { return row_dot_ldq(dim, f16rows); }
// Queries of one group: up to IVF_NQ, fewer when their rows pass the LDS; 0: not even one fits
static int ivf_group(int dim, bool f16rows) {
    const size_t fit = IVF_LDS / ((size_t)ivf_ldq(dim, f16rows) * sizeof(float));
    return (int)(fit < (size_t)IVF_NQ ? fit : (size_t)IVF_NQ);
}
// Work items at most while every n_q <= cap: sum_l cdiv(p_l, nq) * cdiv(len_l, CHUNK) <= sum_l p_l * (len_l / CHUNK + 1)
// = (sum_q n_q) / CHUNK + Q * nprobe
static i64 ivf_max_work(i64 Q, int nprobe, i64 cap) { return Q * cap / IVF_CHUNK + Q * nprobe; }

struct IvfWs {
    unsigned* flag; void* query; i64* poff; i64* pord; i64* base; i64* nfill; i64* wstart; i64* n_work; int4* items; void* members;
    size_t total;
};
// query_bytes: what the scan reads of the Q queries (fp32 / fp16 rows: the normalised queries; int8 rows: planes and s_q)
static IvfWs ivf_carve(void* ws, i64 Q, int nprobe, i64 nlist, size_t query_bytes, i64 cap) {
    IvfWs r{};
    WsCarver c(ws);
    const size_t P = (size_t)Q * nprobe;
    r.flag = (unsigned*)c.take(IVF_FLAGS * sizeof(unsigned));
    r.n_work = (i64*)c.take(sizeof(i64));
    r.query = c.take(query_bytes);
    r.poff = (i64*)c.take((size_t)(nlist + 1) * sizeof(i64));
    r.pord = (i64*)c.take(P * sizeof(i64));
    r.base = (i64*)c.take(P * sizeof(i64));
    r.nfill = (i64*)c.take((size_t)Q * sizeof(i64));
    r.wstart = (i64*)c.take((size_t)(nlist + 1) * sizeof(i64));
    r.items = (int4*)c.take((size_t)ivf_max_work(Q, nprobe, cap) * sizeof(int4));
    r.members = c.take(members_ws_bytes((i64)P, nlist));
    r.total = c.total();
    return r;
}
static size_t ivf_query_bytes(i64 Q, int dim) { return (size_t)Q * dim * sizeof(float); }
// int8 rows: the planes [Q][2][lq], then s_q [Q]
static size_t ivf_planes_bytes(i64 Q, int lq) { return (size_t)Q * 2 * lq; }
static size_t ivf_query_bytes_i8(i64 Q, int lq) { return ivf_planes_bytes(Q, lq) + (size_t)Q * sizeof(float); }
// Queries of one group over int8 rows: up to IVF_NQ_I8, fewer when their planes pass the LDS; 0: not even one fits
static int ivf_group_i8(int lq) {
    const size_t fit = IVF_LDS / ((size_t)2 * lq);
    return (int)(fit < (size_t)IVF_NQ_I8 ? fit : (size_t)IVF_NQ_I8);
}

// What both entries check of the shape; true when it is one a scan can run
static bool ivf_shape_ok(i64 Q, int nprobe, i64 nlist, int dim, i64 cap) {
    return dim >= 1 && ivf_lists_shape_ok(Q, nprobe, nlist, cap);
}

static int ivf_grid() {                        // workgroups of the scan: eight per CU (32 waves)
    static int cus[MI355_MAX_DEVICES] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MI355_MAX_DEVICES) return 256 * 8;
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        cus[dev] = n;
    }
    return cus[dev] * 8;
}

// What the two entries give the pipeline beside their own query side and rows
struct IvfLists {
    i64 Q, G;
    const int64_t *offsets, *order, *probes;
    i64 nlist;
    int nprobe;
    i64 cap, idx_offset;
    float* cand_val;
    int64_t* cand_idx;
    const RankFilter* filt;                    // nullptr: unfiltered
};

// Both entries behind their argument checks.  `a` holds the entry's rows, dim, ldq and nq; prepare(st) queues what makes the
// query side the scan reads; scan(grid, st, a) launches the entry's k_ivf_scan on the filled arguments.
template <class Prepare, class Scan>
static int ivf_run(const char* who, IvfArgs a, const IvfLists& L, const IvfWs& w, hipStream_t st, Prepare prepare, Scan scan) {
    RoctxRange range("ivf/scan");
    MI355_CHECK_HIP(hipMemsetAsync(w.flag, 0, IVF_FLAGS * sizeof(unsigned), st));
    if (int e = prepare(st)) return e;
    const unsigned* members_flag = nullptr;
    if (int e = members_async(L.probes, L.Q * L.nprobe, L.nlist, (int64_t*)w.poff, (int64_t*)w.pord, w.members, st, &members_flag))
        return e;

    a.G = L.G;
    a.offsets = (const i64*)L.offsets; a.order = (const i64*)L.order; a.nlist = L.nlist;
    a.probes = (const i64*)L.probes; a.Q = L.Q; a.nprobe = L.nprobe;
    a.cap = L.cap; a.idx_offset = L.idx_offset;
    a.poff = w.poff; a.pord = w.pord; a.base = w.base; a.nfill = w.nfill; a.wstart = w.wstart; a.items = w.items;
    a.max_work = ivf_max_work(L.Q, L.nprobe, L.cap); a.n_work = w.n_work;
    a.cand_val = L.cand_val; a.cand_idx = (i64*)L.cand_idx; a.flag = w.flag;
    if (L.filt) a.filt = *L.filt;
    a.filtered = L.filt != nullptr;

    hipLaunchKernelGGL(k_ivf_bases, dim3((unsigned)cdiv(L.Q, 256)), dim3(256), 0, st, a);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ivf_plan, dim3(1), dim3(1024), 0, st, a);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ivf_items, dim3((unsigned)L.nlist), dim3(256), 0, st, a);
    MI355_LAUNCH_CHECK();
    const i64 pad_wgs = (L.Q * L.cap + 255) / 256;
    hipLaunchKernelGGL(k_ivf_pad, dim3((unsigned)(pad_wgs < 65535 * 16 ? pad_wgs : 65535 * 16)), dim3(256), 0, st, a);
    MI355_LAUNCH_CHECK();
    scan(dim3((unsigned)ivf_grid()), st, a);
    MI355_LAUNCH_CHECK();

    return ivf_check_flags(w.flag, members_flag, L.nlist, L.G, L.cap, who, st);
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_ivf_scan_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int64_t cap) {
    if (!ivf_shape_ok(Q, nprobe, nlist, dim, cap)) return 0;
    return ivf_carve(nullptr, Q, nprobe, nlist, ivf_query_bytes(Q, dim), cap).total;
}

int mi355_ivf_scan(const float* queries, int64_t Q, int dim, float eps, const void* rows, int rows_dtype, int64_t ld, int64_t G,
                   const int64_t* offsets, const int64_t* order, int64_t nlist, const int64_t* probes, int nprobe, int64_t cap,
                   int64_t idx_offset, const mi355_rank_filter* filter, float* cand_val, int64_t* cand_idx, void* workspace,
                   size_t workspace_bytes, void* stream) {
    const char* who = "ivf_scan";
    MI355_REQUIRE(Q >= 0, "%s: Q=%lld must be >= 0", who, (long long)Q);
    MI355_REQUIRE(rows_dtype == MI355_DTYPE_F32 || rows_dtype == MI355_DTYPE_F16, "%s: unknown rows dtype %d", who, rows_dtype);
    const bool f16rows = rows_dtype == MI355_DTYPE_F16;
    MI355_REQUIRE(dim >= 1, "%s: dim=%d must be >= 1", who, dim);
    MI355_REQUIRE(G >= 1, "%s: G=%lld must be >= 1", who, (long long)G);
    MI355_REQUIRE(ld >= dim, "%s: ld=%lld < dim=%d", who, (long long)ld, dim);
    MI355_REQUIRE(nlist >= 1 && nlist <= IVF_MAX_WGS, "%s: nlist=%lld outside [1, 2^24)", who, (long long)nlist);
    MI355_REQUIRE(nprobe >= 1 && nprobe <= nlist, "%s: nprobe=%d outside [1, nlist=%lld]", who, nprobe, (long long)nlist);
    MI355_REQUIRE(cap >= 1, "%s: cap=%lld must be >= 1", who, (long long)cap);
    RankFilter filt{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &filt)) return e;
    if (Q == 0) return OK;
    MI355_REQUIRE(queries && rows && offsets && order && probes && cand_val && cand_idx,
                  "%s: null queries/rows/offsets/order/probes/candidates pointer", who);
    MI355_REQUIRE(!f16rows || (((uintptr_t)rows & 15) == 0 && ld % 8 == 0),
                  "%s: fp16 rows must be 16-byte aligned with ld=%lld a multiple of 8", who, (long long)ld);
    const int nq = ivf_group(dim, f16rows);
    MI355_REQUIRE(nq >= 1, "%s: dim=%d too large: one query of %d floats does not fit in %zu bytes of LDS", who, dim,
                  ivf_ldq(dim, f16rows), IVF_LDS);
    MI355_REQUIRE(ivf_shape_ok(Q, nprobe, nlist, dim, cap), "%s: shape too large Q=%lld nprobe=%d cap=%lld: Q * nprobe >= 2^31 or "
                  "Q * cap > 2^40", who, (long long)Q, nprobe, (long long)cap);
    const IvfWs w = ivf_carve(workspace, Q, nprobe, nlist, ivf_query_bytes(Q, dim), cap);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);

    IvfArgs a{};
    a.qn = (const float*)w.query; a.rows = rows; a.ld = ld; a.dim = dim; a.ldq = ivf_ldq(dim, f16rows); a.nq = nq;
    const IvfLists L{Q, G, offsets, order, probes, nlist, nprobe, cap, idx_offset, cand_val, cand_idx, filter ? &filt : nullptr};
    const size_t lds = (size_t)nq * a.ldq * sizeof(float);
    const bool vec = ld % 4 == 0 && dim % 4 == 0 && ((uintptr_t)rows & 15) == 0;
    return ivf_run(
        who, a, L, w, (hipStream_t)stream,
        [&](hipStream_t) -> int { return mi355_l2_normalize_rows(queries, (float*)w.query, Q, dim, eps, stream); },
        [&](dim3 grid, hipStream_t st, const IvfArgs& args) {
            if (f16rows)
                hipLaunchKernelGGL((k_ivf_scan<FloatRows<true, true>>), grid, dim3(256), lds, st, args);
            else if (vec)
                hipLaunchKernelGGL((k_ivf_scan<FloatRows<false, true>>), grid, dim3(256), lds, st, args);
            else
                hipLaunchKernelGGL((k_ivf_scan<FloatRows<false, false>>), grid, dim3(256), lds, st, args);
        });
}

size_t mi355_ivf_scan_i8_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int64_t cap) {
    if (!ivf_shape_ok(Q, nprobe, nlist, dim, cap) || dim > I8_MAX_DIM || ivf_group_i8(i8_ld(dim)) < 1) return 0;
    return ivf_carve(nullptr, Q, nprobe, nlist, ivf_query_bytes_i8(Q, i8_ld(dim)), cap).total;
}

int mi355_ivf_scan_i8(const float* queries, int64_t Q, int dim, float eps, const void* codes, const float* scales, int64_t ld,
                      int64_t G, const int64_t* offsets, const int64_t* order, int64_t nlist, const int64_t* probes, int nprobe,
                      int64_t cap, int64_t idx_offset, const mi355_rank_filter* filter, float* cand_val, int64_t* cand_idx,
                      void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ivf_scan_i8";
    MI355_REQUIRE(Q >= 0, "%s: Q=%lld must be >= 0", who, (long long)Q);
    MI355_REQUIRE(dim >= 1 && dim <= I8_MAX_DIM, "%s: dim=%d outside [1, %d]", who, dim, I8_MAX_DIM);
    const int lq = i8_ld(dim), nq = ivf_group_i8(lq);
    MI355_REQUIRE(nq >= 1, "%s: dim=%d too large: one query of %d bytes does not fit in %zu bytes of LDS", who, dim, 2 * lq, IVF_LDS);
    MI355_REQUIRE(G >= 1, "%s: G=%lld must be >= 1", who, (long long)G);
    MI355_REQUIRE(ld >= dim && ld % I8_KSTEP == 0, "%s: ld=%lld must be a multiple of %d and >= dim=%d", who, (long long)ld, I8_KSTEP,
                  dim);
    MI355_REQUIRE(nlist >= 1 && nlist <= IVF_MAX_WGS, "%s: nlist=%lld outside [1, 2^24)", who, (long long)nlist);
    MI355_REQUIRE(nprobe >= 1 && nprobe <= nlist, "%s: nprobe=%d outside [1, nlist=%lld]", who, nprobe, (long long)nlist);
    MI355_REQUIRE(cap >= 1, "%s: cap=%lld must be >= 1", who, (long long)cap);
    RankFilter filt{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &filt)) return e;
    if (Q == 0) return OK;
    MI355_REQUIRE(queries && codes && scales && offsets && order && probes && cand_val && cand_idx,
                  "%s: null queries/codes/scales/offsets/order/probes/candidates pointer", who);
    MI355_REQUIRE(((uintptr_t)codes & 15) == 0, "%s: codes must be 16-byte aligned", who);
    MI355_REQUIRE(ivf_shape_ok(Q, nprobe, nlist, dim, cap), "%s: shape too large Q=%lld nprobe=%d cap=%lld: Q * nprobe >= 2^31 or "
                  "Q * cap > 2^40", who, (long long)Q, nprobe, (long long)cap);
    const IvfWs w = ivf_carve(workspace, Q, nprobe, nlist, ivf_query_bytes_i8(Q, lq), cap);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);

    signed char* planes = (signed char*)w.query;
    float* sq = reinterpret_cast<float*>(planes + ivf_planes_bytes(Q, lq));
    IvfArgs a{};
    a.planes = (const i32x4*)planes; a.sq = sq; a.scales = scales; a.rows = codes; a.ld = ld; a.dim = dim; a.ldq = lq; a.nq = nq;
    const IvfLists L{Q, G, offsets, order, probes, nlist, nprobe, cap, idx_offset, cand_val, cand_idx, filter ? &filt : nullptr};
    const size_t lds = (size_t)nq * 2 * lq;
    return ivf_run(
        who, a, L, w, (hipStream_t)stream,
        [&](hipStream_t st) -> int {
            hipLaunchKernelGGL(k_ivf_queries_i8, dim3((unsigned)cdiv(Q, 4)), dim3(256), 0, st, queries, planes, sq, (i64)Q, dim, lq,
                               eps, vec_ok(queries, dim));
            MI355_LAUNCH_CHECK();
            return OK;
        },
        [&](dim3 grid, hipStream_t st, const IvfArgs& args) {
            hipLaunchKernelGGL((k_ivf_scan<Int8Rows>), grid, dim3(256), lds, st, args);
        });
}

}  // extern "C"
