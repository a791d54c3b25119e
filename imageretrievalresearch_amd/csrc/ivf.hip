// Inverted-file (IVF) search: the scan of the lists a query probes (mi355_ivf_scan).  The gallery's rows are read where they
// lie, through the lists' CSR (offsets, order); the candidates of every query go to a slab that mi355_merge_topk selects
// from.  Nothing is read back to the host between the steps:
//   1. the queries are normalised (mi355_l2_normalize_rows);
//   2. the (query, list) pairs are grouped by list: the kernels of mi355_cluster_members over the flattened probes;
//   3. k_ivf_bases: per query the running sum of its probed lists' lengths = the slot base of each pair, and n_q;
//   4. k_ivf_plan / k_ivf_items: the work items (list, group of up to NQ pairs, chunk of IVF_CHUNK rows) and their count;
//   5. k_ivf_pad: the slots n_q .. cap - 1 of every query;
//   6. k_ivf_scan: a fixed grid loops over the items; one wave per row, the group's queries in LDS.
// Every slot is written by exactly one wave (of k_ivf_scan below n_q, of k_ivf_pad from n_q on).  gfx950 only.
#include "ivf_lists.h"
#include "row_dot.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

constexpr int IVF_NQ = 4;                  // queries of one group at most (k_cos_gemv's count)
constexpr int IVF_CHUNK = 64;              // rows of one work item: 16 per wave
constexpr size_t IVF_LDS = 64 * 1024;      // the group's queries

// What the kernels share
struct IvfArgs {
    const float* qn;        // [Q][dim] normalised queries
    const void* rows;
    i64 ld, G;
    const i64* offsets;     // [nlist + 1]
    const i64* order;       // [G]
    i64 nlist;
    const i64* probes;      // [Q][nprobe]
    i64 Q;
    int nprobe, dim, ldq, nq;      // ldq: floats of one query in LDS (dim rounded up to a unit); nq: queries of a group
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

// The rows [r0, r1) of list l (whose rows begin at order[lb]) against the NQ pairs pord[p0 ..): wave w takes rows r0 + w,
// r0 + w + 4, ...; lane i < NQ writes the slot of pair i.
template <int NQ, bool F16, bool VEC>
__device__ __forceinline__ void scan_chunk(const IvfArgs& a, const float* __restrict__ qs, i64 p0, i64 lb, i64 r0, i64 r1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 myq = 0, mybase = 0, lab = 0, ex = -1;
    if (lane < NQ) {
        const i64 pair = a.pord[p0 + lane];
        myq = pair / a.nprobe;
        mybase = a.base[pair];
        if (a.filtered) query_filter(a.filt, myq, lab, ex);
    }
    for (i64 r = r0 + wave; r < r1; r += 4) {
        const i64 g = a.order[r];
        const bool ok = g >= 0 && g < a.G;                          // the same for the whole wave
        float acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
        if (ok) row_dot<NQ, F16, VEC>(a, g, qs, lane, acc);
        else if (lane == 0) a.flag[IVF_FLAG_ENTRY] = 1u;
        float mine = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float t = wave_sum(acc[q]);
            if (lane == q) mine = t;
        }
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
    }
}

template <bool F16, bool VEC>
__global__ __launch_bounds__(256) void k_ivf_scan(IvfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float qs[];     // [nq][ldq]
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
        for (int i = threadIdx.x; i < n * a.ldq; i += 256) {
            const int qi = i / a.ldq, e = i - qi * a.ldq;
            const i64 q = a.pord[p0 + qi] / a.nprobe;
            qs[i] = e < a.dim ? a.qn[q * a.dim + e] : 0.f;
        }
        __syncthreads();
        switch (n) {                                                // the same for the whole workgroup
            case 1: scan_chunk<1, F16, VEC>(a, qs, p0, lb, r0, r1); break;
            case 2: scan_chunk<2, F16, VEC>(a, qs, p0, lb, r0, r1); break;
            case 3: scan_chunk<3, F16, VEC>(a, qs, p0, lb, r0, r1); break;
            case 4: scan_chunk<4, F16, VEC>(a, qs, p0, lb, r0, r1); break;
            default: break;
        }
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
    unsigned* flag; float* qn; i64* poff; i64* pord; i64* base; i64* nfill; i64* wstart; i64* n_work; int4* items; void* members;
    size_t total;
};
static IvfWs ivf_carve(void* ws, i64 Q, int nprobe, i64 nlist, int dim, i64 cap) {
    IvfWs r{};
    WsCarver c(ws);
    const size_t P = (size_t)Q * nprobe;
    r.flag = (unsigned*)c.take(IVF_FLAGS * sizeof(unsigned));
    r.n_work = (i64*)c.take(sizeof(i64));
    r.qn = (float*)c.take((size_t)Q * dim * sizeof(float));
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

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_ivf_scan_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int64_t cap) {
    if (!ivf_shape_ok(Q, nprobe, nlist, dim, cap)) return 0;
    return ivf_carve(nullptr, Q, nprobe, nlist, dim, cap).total;
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
    const IvfWs w = ivf_carve(workspace, Q, nprobe, nlist, dim, cap);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);

    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("ivf/scan");
    MI355_CHECK_HIP(hipMemsetAsync(w.flag, 0, IVF_FLAGS * sizeof(unsigned), st));
    if (int e = mi355_l2_normalize_rows(queries, w.qn, Q, dim, eps, stream)) return e;
    const unsigned* members_flag = nullptr;
    if (int e = members_async(probes, Q * nprobe, nlist, (int64_t*)w.poff, (int64_t*)w.pord, w.members, st, &members_flag)) return e;

    IvfArgs a{};
    a.qn = w.qn; a.rows = rows; a.ld = ld; a.G = G;
    a.offsets = (const i64*)offsets; a.order = (const i64*)order; a.nlist = nlist;
    a.probes = (const i64*)probes; a.Q = Q; a.nprobe = nprobe; a.dim = dim; a.ldq = ivf_ldq(dim, f16rows); a.nq = nq;
    a.cap = cap; a.idx_offset = idx_offset;
    a.poff = w.poff; a.pord = w.pord; a.base = w.base; a.nfill = w.nfill; a.wstart = w.wstart; a.items = w.items;
    a.max_work = ivf_max_work(Q, nprobe, cap); a.n_work = w.n_work;
    a.cand_val = cand_val; a.cand_idx = (i64*)cand_idx; a.flag = w.flag;
    a.filt = filt; a.filtered = filter != nullptr;

    hipLaunchKernelGGL(k_ivf_bases, dim3((unsigned)cdiv(Q, 256)), dim3(256), 0, st, a);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ivf_plan, dim3(1), dim3(1024), 0, st, a);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ivf_items, dim3((unsigned)nlist), dim3(256), 0, st, a);
    MI355_LAUNCH_CHECK();
    const i64 pad_wgs = (Q * cap + 255) / 256;
    hipLaunchKernelGGL(k_ivf_pad, dim3((unsigned)(pad_wgs < 65535 * 16 ? pad_wgs : 65535 * 16)), dim3(256), 0, st, a);
    MI355_LAUNCH_CHECK();
    const size_t lds = (size_t)nq * a.ldq * sizeof(float);
    const dim3 grid((unsigned)ivf_grid());
    if (f16rows)
        hipLaunchKernelGGL((k_ivf_scan<true, true>), grid, dim3(256), lds, st, a);
    else if (ld % 4 == 0 && dim % 4 == 0 && ((uintptr_t)rows & 15) == 0)
        hipLaunchKernelGGL((k_ivf_scan<false, true>), grid, dim3(256), lds, st, a);
    else
        hipLaunchKernelGGL((k_ivf_scan<false, false>), grid, dim3(256), lds, st, a);
    MI355_LAUNCH_CHECK();

    return ivf_check_flags(w.flag, members_flag, nlist, G, cap, who, st);
}

}  // extern "C"
