// IVF-PQ search (mi355_ivfpq_search): the table scan of pq.hip over the rows of the lists a query probes only.  The index keeps
// a list-ordered copy of the codes (list_codes[p] = codes[order[p]]), so a list is one contiguous byte range and the scan's
// code loads are those of k_pq_scan.  The contract is in include/mi355_retrieval.h: a score is the PQ score, bit for bit, and
// ties go to the lower GALLERY row, whatever the order the lists are scanned in.  Per block of PQ_QBLOCK queries:
//   1. mi355_l2_normalize_rows, k_pq_table (pq.hip): the queries' tables;
//   2. k_ivfpq_bases: per query base[0 .. nprobe] = the running sum of its probed lists' lengths (base[nprobe] = n_q) and
//      lbeg[j] = where list j begins in list order; raises the flags for bad lists and n_q > cap;
//   3. k_ivfpq_scan (k <= 8): workgroup (c, q) owns positions [c * CHUNK, min((c + 1) * CHUNK, n_q)) of query q's concatenated
//      lists and selects k candidates inside (rank_topk_small.inc), merged by topk_select; or
//      k_ivfpq_cands (8 < k <= 1024): the same walk, every position's (value, index) written to a (queries, cap) slab that
//      topk_select (the selection of mi355_merge_topk) reads.
// A workgroup whose chunk begins at or after n_q writes its pads and returns before it touches the table: the grid is sized by
// the host's bound cap, and most workgroups of a short query do nothing.  No atomics: every output slot has one writer.
// One flag read-back (one host sync) after the last launch.
// Residual IVF-PQ (mi355_ivfpq_residual_search, RES below): the codes describe row - centroids[list], so the value of a position
// is coarse[j] + the lookups, j the probe whose list the cursor is in.  k_ivfpq_coarse writes coarse[q][j] = qn_q .
// centroids[probes[q][j]] (row_dot.h, the routine of mi355_rescore_candidates: the same bits) before the scan, which stages the
// query's nprobe terms in LDS behind base[].  mi355_ivfpq_residuals makes the rows the codes are made from.  gfx950 only.
#include "pq_scan.h"
#include "ivf_lists.h"
#include "row_dot.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

constexpr int IVFPQ_CHUNK = 2048;           // positions of one scan workgroup, as PQ_CHUNK: the table load is 1/8 of its lookups
constexpr int IVFPQ_MAX_NPROBE = 1024;      // base[] of one query in LDS: 8 KB + 8 bytes beside the table
constexpr size_t IVFPQ_MAX_LDS = (size_t)PQ_MAX_M * 1024 + (IVFPQ_MAX_NPROBE + 1) * sizeof(i64);
// (residual search: the query's coarse terms behind base[], 4 * nprobe bytes more - 143,368 bytes at M = 128, nprobe = 1024)
constexpr size_t IVFRPQ_MAX_LDS = IVFPQ_MAX_LDS + IVFPQ_MAX_NPROBE * sizeof(float);
constexpr int COARSE_CHUNK = 64;            // (query, list) pairs of one k_ivfpq_coarse workgroup: 16 per wave
constexpr int RESID_ROWS = 4;               // rows of one k_ivfpq_residuals workgroup: one wave each
constexpr i64 IVFPQ_SLAB_BYTES = PQ_SLAB_FLOATS * 4;     // the candidate slab of one query block: the bound of pq_query_block

// What the scan kernels read of one block of queries
struct IvfPqArgs {
    const float* T;                 // [queries][M][256]
    const unsigned char* list_codes;
    const i64* order;               // [G]
    i64 G;
    int M, nprobe, k;
    const i64* base;                // [queries][nprobe + 1]
    const i64* lbeg;                // [queries][nprobe]
    const float* coarse;            // [queries][nprobe]: the residual search's q . centroid terms; not read otherwise
    i64 cap, idx_offset;
    float* ov;                      // k <= 8: [queries][chunks][k]; k > 8: [queries][cap]
    i64* oi;
    unsigned* flag;                 // [IVF_FLAGS]
    RankFilter flt;
};

// base[q][j] = the rows of probes[q][0 .. j), base[q][nprobe] = n_q; lbeg[q][j] = offsets[probes[q][j]].  A list id outside
// [0, nlist) or a list whose offsets do not ascend within [0, G] counts as empty, so the scan never visits it.  One thread per
// query.
__global__ __launch_bounds__(256) void k_ivfpq_bases(const i64* __restrict__ probes, i64 Q, int nprobe, const i64* __restrict__ offsets,
                                                     i64 nlist, i64 G, i64 cap, i64* __restrict__ base, i64* __restrict__ lbeg,
                                                     unsigned* flag) {
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    i64 run = 0;
    bool bad = false;
    for (int j = 0; j < nprobe; ++j) {
        const i64 l = probes[q * nprobe + j];
        i64 b = 0, e = 0;
        if (l < 0 || l >= nlist) bad = true;
        else if (!list_range(offsets, l, G, b, e)) bad = true;
        base[q * (nprobe + 1) + j] = run;
        lbeg[q * nprobe + j] = b;
        run += e - b;
    }
    base[q * (nprobe + 1) + nprobe] = run;
    if (bad) flag[IVF_FLAG_ENTRY] = 1u;
    if (run > cap) flag[IVF_FLAG_CAP] = 1u;
}

// Where position p of a query's concatenated lists lies: list j of its probes holds the positions [sb[j], sb[j + 1]) and begins
// at lbeg[j] in list order.  A thread's positions ascend, so after the binary search of its first one the cursor only moves
// forward.  p < sb[nprobe] = n_q always.
struct ListCursor {
    int j;
    i64 hi, shift;                  // sb[j + 1]; lbeg[j] - sb[j]: the slot of p is p + shift
};
__device__ __forceinline__ void cursor_set(ListCursor& c, const i64* sb, const i64* __restrict__ lbeg, int j) {
    c.j = j;
    c.hi = sb[j + 1];
    c.shift = lbeg[j] - sb[j];
}
__device__ __forceinline__ void cursor_seek(ListCursor& c, const i64* sb, const i64* __restrict__ lbeg, int nprobe, i64 p) {
    int lo = 0, hi = nprobe - 1;                                    // the last j with sb[j] <= p: its list is not empty
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sb[mid] <= p) lo = mid; else hi = mid - 1;
    }
    cursor_set(c, sb, lbeg, lo);
}
__device__ __forceinline__ i64 cursor_slot(ListCursor& c, const i64* sb, const i64* __restrict__ lbeg, i64 p) {
    if (p >= c.hi) {
        int j = c.j + 1;
        while (sb[j + 1] <= p) ++j;                                 // (empty lists in between)
        cursor_set(c, sb, lbeg, j);
    }
    return p + c.shift;
}

// The query's n_q (at most cap) and, unless the chunk is empty, its base[] into sb, its table into tab and (RES) its coarse
// terms into sc; false: empty chunk.  The term of a bad list id is staged but never read: the list counts as empty.
template <int NT, bool RES>
__device__ __forceinline__ bool ivfpq_stage(const IvfPqArgs& a, float* tab, i64*& sb, const float*& sc, i64& nq) {
    const i64* gb = a.base + (i64)blockIdx.y * (a.nprobe + 1);
    nq = gb[a.nprobe] < a.cap ? gb[a.nprobe] : a.cap;               // n_q > cap: flagged by k_ivfpq_bases
    if ((i64)blockIdx.x * IVFPQ_CHUNK >= nq) return false;          // the same for the whole workgroup
    sb = reinterpret_cast<i64*>(tab + (size_t)a.M * PQ_CENTROIDS);
    for (int i = threadIdx.x; i <= a.nprobe; i += NT) sb[i] = gb[i];
    if constexpr (RES) {                                            // coarse[] of the query behind base[]
        float* c = reinterpret_cast<float*>(sb + a.nprobe + 1);
        const float* gc = a.coarse + (i64)blockIdx.y * a.nprobe;
        for (int i = threadIdx.x; i < a.nprobe; i += NT) c[i] = gc[i];
        sc = c;
    }
    pq_load_table<NT>(tab, a.T, a.M);                               // (ends in the barrier that covers sb too)
    return true;
}

// ---- scan with the selection inside (k <= K <= 8): grid (cdiv(cap, IVFPQ_CHUNK), queries).  The body is the small-k selection
// of the score slabs; its candidate value is the lookups of the code row at the position's slot, its row the list's entry
// there.  ov / oi [queries][chunks][k].
template <int K, bool FILT, bool VEC, int NT, bool RES>
__global__ __launch_bounds__(NT) void k_ivfpq_scan(IvfPqArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tab[];    // [M][256], base[] of the query [nprobe + 1] i64, RES: coarse[nprobe]
    const int k = a.k;
    float* const ov = a.ov;
    i64* const oi = a.oi;
    i64* sb = nullptr;
    const float* sc = nullptr;
    i64 nq = 0;
    if (!ivfpq_stage<NT, RES>(a, tab, sb, sc, nq)) {
        const i64 o = ((i64)blockIdx.y * gridDim.x + blockIdx.x) * k;
        if ((int)threadIdx.x < k) { ov[o + threadIdx.x] = NEG_INF; oi[o + threadIdx.x] = IDX_PAD; }
        return;
    }
    const i64* const lbeg = a.lbeg + (i64)blockIdx.y * a.nprobe;
    ListCursor cur{0, 0, 0};
    const i64 first = (i64)blockIdx.x * IVFPQ_CHUNK + threadIdx.x;
    if (first < nq) cursor_seek(cur, sb, lbeg, a.nprobe, first);
    i64 slot = 0, grow = 0;
    bool gbad = false;
    // the code row's slot, then the gallery row it came from (0 for an entry outside the gallery: skipped and flagged)
    auto visit = [&](i64 p) {
        slot = cursor_slot(cur, sb, lbeg, p);
        grow = a.order[slot];
        gbad = grow < 0 || grow >= a.G;
        if (gbad) { grow = 0; a.flag[IVF_FLAG_ENTRY] = 1u; }
    };
    const float* const vals = nullptr;
    const i64* const idxs = nullptr;
    const int* const idxs32 = nullptr;
    const i64 rowlen = nq, in_stride = 0, chunk_len = IVFPQ_CHUNK, idx_offset = a.idx_offset;
    const RankFilter& flt = a.flt;
    // (RES: the cursor stands in the position's list after visit, so sc[cur.j] is the term of the row's own list)
    auto value = [&](i64 p) {
        visit(p);
        const float s = pq_score<VEC>(tab, a.list_codes, slot, a.M);
        if constexpr (RES) return __fadd_rn(sc[cur.j], s);
        else return s;
    };
#define TOPK_SMALL_VALUE(j) ((void)v, value(j))
#define TOPK_SMALL_ROW(j) grow
#define TOPK_SMALL_SKIP(j) gbad
#define TOPK_SMALL_THREADS NT
#include "rank_topk_small.inc"
#undef TOPK_SMALL_THREADS
#undef TOPK_SMALL_SKIP
#undef TOPK_SMALL_ROW
#undef TOPK_SMALL_VALUE
}

// ---- the candidate slab (8 < k): the same grid and walk; slot p of query q holds (score, row + idx_offset), or "no
// candidate" (-inf, 2^62) for an ineligible row, a bad entry and every position from n_q on.  ov / oi [queries][cap].
template <bool FILT, bool VEC, int NT, bool RES>
__global__ __launch_bounds__(NT) void k_ivfpq_cands(IvfPqArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tab[];    // [M][256], base[] of the query [nprobe + 1] i64, RES: coarse[nprobe]
    const i64 q = blockIdx.y;
    const i64 c0 = (i64)blockIdx.x * IVFPQ_CHUNK, c1 = c0 + IVFPQ_CHUNK < a.cap ? c0 + IVFPQ_CHUNK : a.cap;
    float* const ov = a.ov + q * a.cap;
    i64* const oi = a.oi + q * a.cap;
    i64* sb = nullptr;
    const float* sc = nullptr;
    i64 nq = 0;
    if (!ivfpq_stage<NT, RES>(a, tab, sb, sc, nq)) {
        for (i64 p = c0 + threadIdx.x; p < c1; p += NT) { ov[p] = NEG_INF; oi[p] = NO_CAND_IDX; }
        return;
    }
    const i64* const lbeg = a.lbeg + q * a.nprobe;
    ListCursor cur{0, 0, 0};
    if (c0 + threadIdx.x < nq) cursor_seek(cur, sb, lbeg, a.nprobe, c0 + threadIdx.x);
    i64 fq_lab = 0, fq_ex = -1;
    if constexpr (FILT) query_filter(a.flt, q, fq_lab, fq_ex);
    for (i64 p = c0 + threadIdx.x; p < c1; p += NT) {
        float x = NEG_INF;
        i64 id = NO_CAND_IDX;
        if (p < nq) {
            const i64 slot = cursor_slot(cur, sb, lbeg, p);
            const i64 g = a.order[slot];
            bool ok = g >= 0 && g < a.G;
            if (!ok) a.flag[IVF_FLAG_ENTRY] = 1u;
            if constexpr (FILT) {
                if (ok) ok = eligible(a.flt.mode, fq_lab, a.flt.mode != MI355_LABEL_ANY ? a.flt.glab[g] : 0, fq_ex, g);
            }
            if (ok) {
                x = pq_score<VEC>(tab, a.list_codes, slot, a.M);
                if constexpr (RES) x = __fadd_rn(sc[cur.j], x);
                id = g + a.idx_offset;
            }
        }
        ov[p] = x;
        oi[p] = id;
    }
}

// ---- the coarse terms of the residual search: grid (cdiv(nprobe, COARSE_CHUNK), queries); the normalised query in LDS, wave w
// takes probes w, w + 4, ... of the chunk: coarse[q][j] = qn_q . centroids[probes[q][j]], one wave per pair as k_rescore (pq.hip)
// scores a candidate.  A list id outside [0, nlist) reads nothing and gets -inf; k_ivfpq_bases flags it and makes its list empty.
struct CoarseArgs {
    const float* qn;        // [queries][dim] normalised
    const float* rows;      // centroids [nlist][dim]
    i64 ld, nlist;
    int dim, ldq, nprobe;
    const i64* probes;      // [queries][nprobe]
    float* out;             // [queries][nprobe]
};
template <bool VEC>
__global__ __launch_bounds__(256) void k_ivfpq_coarse(CoarseArgs a) {
    extern __shared__ __attribute__((aligned(16))) float qs[];     // [ldq]
    const i64 q = blockIdx.y;
    for (int i = threadIdx.x; i < a.ldq; i += 256) qs[i] = i < a.dim ? a.qn[q * a.dim + i] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j0 = blockIdx.x * COARSE_CHUNK, j1 = j0 + COARSE_CHUNK < a.nprobe ? j0 + COARSE_CHUNK : a.nprobe;
    for (int j = j0 + wave; j < j1; j += 4) {
        const i64 l = a.probes[q * a.nprobe + j];
        const bool ok = l >= 0 && l < a.nlist;                      // the same for the whole wave
        float acc[1] = {0.f};
        if (ok) row_dot<1, false, VEC>(a, l, qs, lane, acc);
        const float t = wave_sum(acc[0]);
        if (lane == 0) a.out[q * a.nprobe + j] = ok ? t : NEG_INF;
    }
}

// ---- residual rows: out[r] = n[r] - centroids[assign[r]], one fp32 subtraction per element; one wave per row, 16 bytes per
// lane and load where dim % 4 == 0 (VEC).  n and out may be the same buffer (each element is read, then written, by one lane).
// A row whose assignment falls outside [0, nlist) is left unwritten and raises the flag.
template <bool VEC>
__global__ __launch_bounds__(64 * RESID_ROWS) void k_ivfpq_residuals(const float* n, i64 R, int dim, const i64* __restrict__ assign,
                                                                     const float* __restrict__ centroids, i64 nlist, float* out,
                                                                     unsigned* flag) {
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * RESID_ROWS + (threadIdx.x >> 6);
    if (r >= R) return;
    const i64 l = assign[r];
    if (l < 0 || l >= nlist) {
        if (lane == 0) *flag = 1u;
        return;
    }
    const float* x = n + r * dim;
    const float* c = centroids + l * dim;
    float* o = out + r * dim;
    if constexpr (VEC) {
        for (int u = lane; u < dim / 4; u += 64) {
            const f32x4 a = reinterpret_cast<const f32x4*>(x)[u], b = reinterpret_cast<const f32x4*>(c)[u];
            f32x4 d;
            d.x = __fsub_rn(a.x, b.x); d.y = __fsub_rn(a.y, b.y); d.z = __fsub_rn(a.z, b.z); d.w = __fsub_rn(a.w, b.w);
            reinterpret_cast<f32x4*>(o)[u] = d;
        }
    } else {
        for (int i = lane; i < dim; i += 64) o[i] = __fsub_rn(x[i], c[i]);
    }
}

// ---- host side
static bool ivfpq_shape_ok(i64 Q, int nprobe, i64 nlist, int dim, int M, i64 G, i64 cap, int k) {
    return G >= 1 && G <= ((i64)1 << 40) && pq_shape_ok(dim, M) && ivf_lists_shape_ok(Q, nprobe, nlist, cap) &&
           nprobe <= IVFPQ_MAX_NPROBE && k >= 1 && k <= LARGE_K && k <= cap;
}
// Queries of one table / scan launch: PQ_QBLOCK, fewer when their candidate slab (k > 8: 12 bytes a slot) would pass the bound
static i64 ivfpq_query_block(i64 Q, i64 cap, int k) {
    i64 qb = PQ_QBLOCK;
    if (k > SMALL_K) {
        const i64 fit = IVFPQ_SLAB_BYTES / (12 * cap);
        if (fit < qb) qb = fit < 1 ? 1 : fit;
    }
    return qb < Q ? qb : Q;
}
// Scratch of a search: the flags, the normalised queries, then per query block its tables, bases and list starts, its candidate
// lists (k <= 8) or slab (k > 8) and the selection's own scratch; the residual search's coarse terms of the block come last, so
// that the plain layout is what it was
struct IvfPqWs {
    unsigned* flag; float* qn; float* T; i64* base; i64* lbeg; float* cand_val; i64* cand_idx; void* topk; size_t topk_bytes;
    float* coarse; size_t total;
};
static IvfPqWs ivfpq_carve(void* ws, i64 Q, int nprobe, int dim, int M, i64 cap, int k, bool res) {
    IvfPqWs r{};
    WsCarver c(ws);
    const i64 qb = ivfpq_query_block(Q, cap, k);
    const i64 slots = k <= SMALL_K ? (i64)cdiv(cap, IVFPQ_CHUNK) * k : cap;
    r.flag = (unsigned*)c.take(IVF_FLAGS * sizeof(unsigned));
    r.qn = (float*)c.take((size_t)Q * dim * sizeof(float));
    r.T = (float*)c.take((size_t)qb * M * PQ_CENTROIDS * sizeof(float));
    r.base = (i64*)c.take((size_t)qb * (nprobe + 1) * sizeof(i64));
    r.lbeg = (i64*)c.take((size_t)qb * nprobe * sizeof(i64));
    r.cand_val = (float*)c.take((size_t)qb * slots * sizeof(float));
    r.cand_idx = (i64*)c.take((size_t)qb * slots * sizeof(i64));
    r.topk_bytes = topk_ws_bytes(qb, slots, k);
    r.topk = c.take(r.topk_bytes);
    if (res) r.coarse = (float*)c.take((size_t)qb * nprobe * sizeof(float));
    r.total = c.total();
    return r;
}

// The scan kernels ask for up to 128 KB + 8 KB (RES: + 4 KB) of dynamic LDS: raise each one's limit once per device
template <bool RES, class Kern>
static int ivfpq_launch(Kern kern, bool* done, dim3 grid, int nt, const IvfPqArgs& a, hipStream_t st) {
    if (first_time_on_this_device(done))
        MI355_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)(RES ? IVFRPQ_MAX_LDS : IVFPQ_MAX_LDS)));
    const size_t lds = (size_t)a.M * 1024 + (size_t)(a.nprobe + 1) * sizeof(i64) + (RES ? (size_t)a.nprobe * sizeof(float) : 0);
    hipLaunchKernelGGL(kern, grid, dim3(nt), lds, st, a);
    MI355_LAUNCH_CHECK();
    return OK;
}
template <int K, bool FILT, bool VEC, int NT, bool RES>
static int launch_scan_one(dim3 grid, const IvfPqArgs& a, hipStream_t st) {
    static bool done[MI355_MAX_DEVICES] = {false};
    return ivfpq_launch<RES>(k_ivfpq_scan<K, FILT, VEC, NT, RES>, done, grid, NT, a, st);
}
template <bool FILT, bool VEC, int NT, bool RES>
static int launch_cands_one(dim3 grid, const IvfPqArgs& a, hipStream_t st) {
    static bool done[MI355_MAX_DEVICES] = {false};
    return ivfpq_launch<RES>(k_ivfpq_cands<FILT, VEC, NT, RES>, done, grid, NT, a, st);
}
template <bool FILT, bool VEC, int NT, bool RES>
static int launch_nt(dim3 grid, const IvfPqArgs& a, hipStream_t st) {
    if (a.k > SMALL_K) return launch_cands_one<FILT, VEC, NT, RES>(grid, a, st);
    if (a.k <= 1) return launch_scan_one<1, FILT, VEC, NT, RES>(grid, a, st);
    if (a.k <= 2) return launch_scan_one<2, FILT, VEC, NT, RES>(grid, a, st);
    if (a.k <= 4) return launch_scan_one<4, FILT, VEC, NT, RES>(grid, a, st);
    return launch_scan_one<8, FILT, VEC, NT, RES>(grid, a, st);
}
template <bool FILT, bool VEC, bool RES>
static int launch_filt_vec(dim3 grid, const IvfPqArgs& a, hipStream_t st) {
    const int nt = pq_threads(a.M);
    if (nt == 256) return launch_nt<FILT, VEC, 256, RES>(grid, a, st);
    if (nt == 512) return launch_nt<FILT, VEC, 512, RES>(grid, a, st);
    return launch_nt<FILT, VEC, 1024, RES>(grid, a, st);
}
template <bool RES>
static int launch_ivfpq(dim3 grid, const IvfPqArgs& a, bool filtered, hipStream_t st) {
    const bool vec = a.M % 16 == 0;
    if (filtered) return vec ? launch_filt_vec<true, true, RES>(grid, a, st) : launch_filt_vec<true, false, RES>(grid, a, st);
    return vec ? launch_filt_vec<false, true, RES>(grid, a, st) : launch_filt_vec<false, false, RES>(grid, a, st);
}

// Both searches: centroids null is the plain one (mi355_ivfpq_search), otherwise the residual one
static int ivfpq_search(const char* who, const float* queries, i64 Q, int dim, float eps, const float* codebooks, int M,
                        const void* list_codes, i64 G, const int64_t* offsets, const int64_t* order, i64 nlist, const int64_t* probes,
                        int nprobe, i64 cap, int k, i64 idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                        void* workspace, size_t workspace_bytes, void* stream, const float* centroids, bool res) {
    MI355_REQUIRE(queries && codebooks && list_codes && offsets && order && probes && out_val && out_idx && (!res || centroids),
                  "%s: null pointer", who);
    MI355_REQUIRE(Q >= 0 && G >= 1 && dim >= 1, "%s: bad shape Q=%lld G=%lld dim=%d", who, (long long)Q, (long long)G, dim);
    if (int e = pq_check_shape(who, dim, M)) return e;
    MI355_REQUIRE(((uintptr_t)list_codes & 15) == 0, "%s: list_codes must be 16-byte aligned", who);
    MI355_REQUIRE(nlist >= 1 && nlist <= IVF_MAX_WGS, "%s: nlist=%lld outside [1, 2^24)", who, (long long)nlist);
    MI355_REQUIRE(nprobe >= 1 && nprobe <= nlist && nprobe <= IVFPQ_MAX_NPROBE, "%s: nprobe=%d outside [1, min(nlist=%lld, %d)]", who,
                  nprobe, (long long)nlist, IVFPQ_MAX_NPROBE);
    MI355_REQUIRE(cap >= 1, "%s: cap=%lld must be >= 1", who, (long long)cap);
    MI355_REQUIRE(k >= 1 && k <= LARGE_K && k <= cap, "%s: k=%d outside [1, %lld] (min(%d, cap))", who, k,
                  (long long)(cap < LARGE_K ? cap : LARGE_K), LARGE_K);
    MI355_REQUIRE(Q <= (((i64)1 << 31) - 1) / nprobe && (Q == 0 || cap <= ((i64)1 << 40) / Q) && G <= ((i64)1 << 40),
                  "%s: shape too large Q=%lld nprobe=%d cap=%lld G=%lld: Q * nprobe >= 2^31, Q * cap > 2^40 or G > 2^40", who,
                  (long long)Q, nprobe, (long long)cap, (long long)G);
    RankFilter fall{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &fall)) return e;
    if (Q == 0) return OK;
    const IvfPqWs w = ivfpq_carve(workspace, Q, nprobe, dim, M, cap, k, res);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);

    hipStream_t st = (hipStream_t)stream;
    const bool fused = k <= SMALL_K;
    RoctxRange range(res ? (fused ? "ivfrpq/coarse + scan + per-chunk top-k" : "ivfrpq/coarse + scan (candidate slab) + top-k")
                         : (fused ? "ivfpq/scan + per-chunk top-k" : "ivfpq/scan (candidate slab) + top-k"));
    MI355_CHECK_HIP(hipMemsetAsync(w.flag, 0, IVF_FLAGS * sizeof(unsigned), st));
    if (int e = mi355_l2_normalize_rows(queries, w.qn, Q, dim, eps, stream)) return e;
    set_rank_path(MI355_RANK_PATH_PQ | (fused ? MI355_RANK_PATH_FUSED : MI355_RANK_PATH_BITONIC));
    const i64 qb = ivfpq_query_block(Q, cap, k), nch = cdiv(cap, IVFPQ_CHUNK), slots = fused ? nch * k : cap;
    for (i64 q0 = 0; q0 < Q; q0 += qb) {
        const i64 qn = Q - q0 < qb ? Q - q0 : qb;
        // (unfiltered: an empty filter, so that the slots the probed lists leave empty end as (-inf, -1) all the same)
        const RankFilter fb = filter ? filter_from(fall, q0) : RankFilter{};
        if (int e = launch_table(w.qn + q0 * dim, qn, dim, codebooks, M, w.T, st)) return e;
        hipLaunchKernelGGL(k_ivfpq_bases, dim3((unsigned)cdiv(qn, 256)), dim3(256), 0, st, (const i64*)probes + q0 * nprobe, qn, nprobe,
                           (const i64*)offsets, (i64)nlist, (i64)G, (i64)cap, w.base, w.lbeg, w.flag);
        MI355_LAUNCH_CHECK();
        IvfPqArgs a{};
        a.T = w.T; a.list_codes = (const unsigned char*)list_codes; a.order = (const i64*)order; a.G = G;
        a.M = M; a.nprobe = nprobe; a.k = k;
        a.base = w.base; a.lbeg = w.lbeg; a.cap = cap; a.idx_offset = idx_offset;
        a.ov = w.cand_val; a.oi = w.cand_idx; a.flag = w.flag; a.flt = fb;
        if (res) {
            // (dim % 4 == 0 by the PQ shape rules; the dot's bits do not depend on the width of the loads)
            const bool cvec = ((uintptr_t)centroids & 15) == 0;
            const CoarseArgs c{w.qn + q0 * dim, centroids, dim, nlist, dim, row_dot_ldq(dim, false), nprobe,
                               (const i64*)probes + q0 * nprobe, w.coarse};
            const dim3 cgrid((unsigned)cdiv(nprobe, COARSE_CHUNK), (unsigned)qn);
            const size_t clds = (size_t)c.ldq * sizeof(float);
            if (cvec) hipLaunchKernelGGL(k_ivfpq_coarse<true>, cgrid, dim3(256), clds, st, c);
            else hipLaunchKernelGGL(k_ivfpq_coarse<false>, cgrid, dim3(256), clds, st, c);
            MI355_LAUNCH_CHECK();
            a.coarse = w.coarse;
        }
        const dim3 grid((unsigned)nch, (unsigned)qn);
        if (int e = res ? launch_ivfpq<true>(grid, a, filter != nullptr, st) : launch_ivfpq<false>(grid, a, filter != nullptr, st))
            return e;
        // the candidates carry their indices: ties resolve on the gallery row, not on the position in the scan
        if (int e = topk_select(w.cand_val, w.cand_idx, qn, slots, slots, k, 0, out_val + q0 * k, (i64*)out_idx + q0 * k, w.topk,
                                w.topk_bytes, st, nullptr, &fb))
            return e;
    }
    return ivf_check_flags(w.flag, nullptr, nlist, G, cap, who, st);
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_ivfpq_search_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int M, int64_t cap, int k) {
    if (!ivfpq_shape_ok(Q, nprobe, nlist, dim, M, 1, cap, k)) return 0;
    return ivfpq_carve(nullptr, Q, nprobe, dim, M, cap, k, false).total;
}

int mi355_ivfpq_search(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M, const void* list_codes,
                       int64_t G, const int64_t* offsets, const int64_t* order, int64_t nlist, const int64_t* probes, int nprobe,
                       int64_t cap, int k, int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return ivfpq_search("ivfpq_search", queries, Q, dim, eps, codebooks, M, list_codes, G, offsets, order, nlist, probes, nprobe, cap, k,
                        idx_offset, filter, out_val, out_idx, workspace, workspace_bytes, stream, nullptr, false);
}

size_t mi355_ivfpq_residual_search_workspace_bytes(int64_t Q, int nprobe, int64_t nlist, int dim, int M, int64_t cap, int k) {
    if (!ivfpq_shape_ok(Q, nprobe, nlist, dim, M, 1, cap, k)) return 0;
    return ivfpq_carve(nullptr, Q, nprobe, dim, M, cap, k, true).total;
}

int mi355_ivfpq_residual_search(const float* queries, int64_t Q, int dim, float eps, const float* codebooks, int M,
                                const void* list_codes, int64_t G, const int64_t* offsets, const int64_t* order, int64_t nlist,
                                const int64_t* probes, int nprobe, int64_t cap, int k, int64_t idx_offset,
                                const mi355_rank_filter* filter, const float* centroids, float* out_val, int64_t* out_idx,
                                void* workspace, size_t workspace_bytes, void* stream) {
    return ivfpq_search("ivfpq_residual_search", queries, Q, dim, eps, codebooks, M, list_codes, G, offsets, order, nlist, probes,
                        nprobe, cap, k, idx_offset, filter, out_val, out_idx, workspace, workspace_bytes, stream, centroids, true);
}

int mi355_ivfpq_residuals(const float* rows, int64_t R, int dim, int rows_are_normalized, float eps, const int64_t* assignments,
                          const float* centroids, int64_t nlist, float* residuals, void* workspace, size_t workspace_bytes,
                          void* stream) {
    const char* who = "ivfpq_residuals";
    MI355_REQUIRE(rows && assignments && centroids && residuals, "%s: null pointer", who);
    MI355_REQUIRE(R >= 0 && R <= ((i64)1 << 31) && dim >= 1 && dim <= PQ_MAX_M * PQ_MAX_DSUB, "%s: bad shape R=%lld dim=%d (R <= 2^31, "
                  "dim <= %d)", who, (long long)R, dim, PQ_MAX_M * PQ_MAX_DSUB);
    MI355_REQUIRE(nlist >= 1 && nlist <= IVF_MAX_WGS, "%s: nlist=%lld outside [1, 2^24)", who, (long long)nlist);
    if (R == 0) return OK;
    MI355_REQUIRE(workspace && workspace_bytes >= MI355_IVFPQ_RESIDUALS_WORKSPACE, "%s: workspace %zu < %d bytes", who, workspace_bytes,
                  MI355_IVFPQ_RESIDUALS_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("ivfrpq/residuals");
    unsigned* flag = (unsigned*)align256(workspace);
    MI355_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), st));
    const float* n = rows;
    if (!rows_are_normalized) {                                     // normalised into the output, the residual taken in place
        if (int e = mi355_l2_normalize_rows(rows, residuals, R, dim, eps, stream)) return e;
        n = residuals;
    }
    const bool vec = dim % 4 == 0 && (((uintptr_t)n | (uintptr_t)centroids | (uintptr_t)residuals) & 15) == 0;
    const dim3 grid((unsigned)cdiv(R, RESID_ROWS));
    if (vec) hipLaunchKernelGGL(k_ivfpq_residuals<true>, grid, dim3(64 * RESID_ROWS), 0, st, n, (i64)R, dim, (const i64*)assignments,
                                centroids, (i64)nlist, residuals, flag);
    else hipLaunchKernelGGL(k_ivfpq_residuals<false>, grid, dim3(64 * RESID_ROWS), 0, st, n, (i64)R, dim, (const i64*)assignments,
                            centroids, (i64)nlist, residuals, flag);
    MI355_LAUNCH_CHECK();
    unsigned bad = 0;
    MI355_CHECK_HIP(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    MI355_REQUIRE(!bad, "%s: an assignment outside [0, nlist=%lld)", who, (long long)nlist);
    return OK;
}

}  // extern "C"
