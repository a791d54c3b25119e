// Graph search: a best-first walk over a gallery's neighbour lists (mi355_graph_search).  One workgroup per query holds in LDS
// the normalised query, the beam (the best ef rows seen so far, sorted in the order of mi355_merge_topk, each with an
// "expanded" bit) and the visited set (an open-addressing table sized per call so that it can never fill).  One hop:
//   1. wave 0 finds the first beam entry not yet expanded, reads its list (one coalesced load of degree int32), enters every
//      neighbour into the visited set and compacts the ones that were new, in list order;
//   2. every wave scores new rows, one wave per row, with the row dot of the IVF scan (row_dot.h): the bits of
//      mi355_rescore_candidates for that (query, row);
//   3. the new rows are merged into the beam by rank: an entry's place is the number of entries better than it (the beam is
//      sorted, the new rows are at most 64), so the result does not depend on the order the new rows were scored in.
// The seeds go through the same three steps as "hop -1" against an empty beam.  Every loop is bounded before it starts
// (max_iters, degree, the table size); no workgroup waits on another; there are no global atomics.  gfx950 only.
#include "ivf_lists.h"
#include "row_dot.h"
#include "../../include/mi355_retrieval.h"

namespace mi355 {

constexpr int GR_THREADS = 1024, GR_WAVES = GR_THREADS / 64;   // one row per wave: 16 rows in flight per workgroup
constexpr int GR_MAX_EF = 512;             // beam entries at most (one thread each in the merge)
constexpr int GR_MAX_LIST = 64;            // neighbours of a row / seeds of a query at most: one lane each
constexpr int GR_MAX_DIM = 4096;
constexpr i64 GR_MAX_VISITS = 16384;       // nseed + max_iters * degree at most: a 128 KB table
constexpr unsigned GR_EMPTY = 0xffffffffu; // a free slot of the visited set (rows are below 2^31)
constexpr unsigned GR_EXPANDED = 0x80000000u;

struct GraphArgs {
    const float* qn;        // [Q][dim] normalised queries
    const void* rows;
    i64 ld, G;
    int dim, ldq;
    const int* graph;       // [G][degree]
    const i64* seeds;       // [Q][nseed]
    int degree, nseed, k, ef, max_iters;
    unsigned tsize;         // slots of the visited set, a power of two
    i64 idx_offset;
    float* out_val;         // [Q][k]
    i64* out_idx;           // [Q][k]
    int* out_iters;         // [Q] or null
    int* out_visited;       // [Q] or null
    unsigned* flag;         // [IVF_FLAGS]
    RankFilter filt;
    bool filtered;
};

// The dynamic LDS of one workgroup, in this order
struct GraphLds {
    size_t qs, bs, br, cand, ns, ctl, tab, total;
};
static inline GraphLds graph_lds(int ldq, int ef, unsigned tsize) {
    GraphLds l{};
    size_t o = 0;
    l.qs = o; o += (size_t)ldq * sizeof(float);                     // the query, zero from dim on (a multiple of 16 bytes)
    l.bs = o; o += (size_t)2 * ef * sizeof(float);                  // the beam's scores, two buffers
    l.br = o; o += (size_t)2 * ef * sizeof(unsigned);               // its rows | GR_EXPANDED
    l.cand = o; o += GR_MAX_LIST * sizeof(int);                     // the new rows of this hop
    l.ns = o; o += GR_MAX_LIST * sizeof(float);                     // their scores
    l.ctl = o; o += 4 * sizeof(int);                                // [0]: how many, -1: the walk is over
    l.tab = o; o += (size_t)tsize * sizeof(unsigned);               // the visited set
    l.total = o;
    return l;
}
// Slots of the visited set: the power of two at or above 2 * (nseed + max_iters * degree)
static inline unsigned graph_table_slots(int nseed, int max_iters, int degree) {
    const i64 need = 2 * ((i64)nseed + (i64)max_iters * degree);
    unsigned t = 8;
    while ((i64)t < need) t <<= 1;
    return t;
}

template <bool F16, bool VEC>
__global__ __launch_bounds__(GR_THREADS) void k_graph_search(GraphArgs a, GraphLds L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qs = reinterpret_cast<float*>(smem + L.qs);
    float* bs = reinterpret_cast<float*>(smem + L.bs);              // [2][ef]
    unsigned* br = reinterpret_cast<unsigned*>(smem + L.br);        // [2][ef]
    int* cand = reinterpret_cast<int*>(smem + L.cand);
    float* ns = reinterpret_cast<float*>(smem + L.ns);
    int* ctl = reinterpret_cast<int*>(smem + L.ctl);
    unsigned* tab = reinterpret_cast<unsigned*>(smem + L.tab);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 q = blockIdx.x;
    const int ef = a.ef;
    const unsigned tmask = a.tsize - 1u;
    const int tshift = 32 - (31 - __builtin_clz(a.tsize));          // the top log2(tsize) bits of the hash

    for (int i = tid; i < a.ldq; i += GR_THREADS) qs[i] = i < a.dim ? a.qn[q * a.dim + i] : 0.f;
    for (unsigned i = tid; i < a.tsize; i += GR_THREADS) tab[i] = GR_EMPTY;
    __syncthreads();

    int nb = 0, cur = 0, iters = 0, visited = 0;
    for (int step = -1; step < a.max_iters; ++step) {              // step -1: the seeds
        if (wave == 0) {
            // 1. the rows this hop offers: lane j holds seed j, or neighbour j of the first unexpanded beam entry
            i64 n = -1;
            bool have = true;
            if (step < 0) {
                if (lane < a.nseed) n = a.seeds[q * a.nseed + lane];
            } else {
                int p = -1;
                for (int c0 = 0; c0 < nb; c0 += 64) {
                    const int i = c0 + lane;
                    const bool open = i < nb && !(br[cur * ef + i] & GR_EXPANDED);
                    const unsigned long long m = __ballot(open);
                    if (m) {
                        p = c0 + __builtin_ctzll(m);
                        break;
                    }
                }
                if (p < 0) {
                    have = false;
                } else {
                    const unsigned row = br[cur * ef + p];             // not expanded: the bare row, inside [0, G)
                    if (lane == 0) br[cur * ef + p] = row | GR_EXPANDED;
                    if (lane < a.degree) n = a.graph[(i64)row * a.degree + lane];
                }
            }
            const bool real = n >= 0 && n < a.G;
            if (n != -1 && !real) a.flag[IVF_FLAG_ENTRY] = 1u;        // never dereferenced
            // the visited set: whoever turns a free slot into the row is the one that found it new
            bool fresh = false;
            if (real) {
                const unsigned key = (unsigned)n;
                unsigned h = (key * 2654435761u) >> tshift;
                for (unsigned t = 0; t < a.tsize; ++t) {
                    const unsigned old = atomicCAS(&tab[h], GR_EMPTY, key);
                    if (old == GR_EMPTY) fresh = true;
                    if (old == GR_EMPTY || old == key) break;
                    h = (h + 1u) & tmask;
                }
            }
            const unsigned long long m = __ballot(fresh);
            if (fresh) cand[__popcll(m & ((1ull << lane) - 1ull))] = (int)n;
            if (lane == 0) ctl[0] = have ? __popcll(m) : -1;
        }
        __syncthreads();
        const int nnew = ctl[0];
        if (nnew < 0) break;                                        // no entry left to expand (the same for every thread)
        if (step >= 0) ++iters;
        visited += nnew;
        if (nnew > 0) {
            // 2. the scores of the new rows
            for (int i = wave; i < nnew; i += GR_WAVES) {
                float acc[1] = {0.f};
                row_dot<1, F16, VEC>(a, (i64)cand[i], qs, lane, acc);
                const float t = wave_sum(acc[0]);
                if (lane == 0) ns[i] = t;
            }
            __syncthreads();
            // 3. beam[cur ^ 1] = the best ef of beam[cur] and the new rows: every entry goes to its rank
            const float* obs = bs + cur * ef;
            const unsigned* obr = br + cur * ef;
            float* nbs = bs + (cur ^ 1) * ef;
            unsigned* nbr = br + (cur ^ 1) * ef;
            if (tid < nb) {                                         // an old entry: its place plus the new rows that beat it
                const float s = obs[tid];
                const unsigned r = obr[tid];
                const i64 row = r & ~GR_EXPANDED;
                int rank = tid;
                for (int j = 0; j < nnew; ++j) rank += better(ns[j], cand[j], s, row) ? 1 : 0;
                if (rank < ef) {
                    nbs[rank] = s;
                    nbr[rank] = r;
                }
            }
            if (tid < nnew) {                                       // a new row: the old entries and the new rows that beat it
                const float s = ns[tid];
                const i64 row = cand[tid];
                int lo = 0, hi = nb;                                // the first old entry that does not beat it
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (better(obs[mid], (i64)(obr[mid] & ~GR_EXPANDED), s, row)) lo = mid + 1; else hi = mid;
                }
                int rank = lo;
                for (int j = 0; j < nnew; ++j) rank += (j != tid && better(ns[j], cand[j], s, row)) ? 1 : 0;
                if (rank < ef) {
                    nbs[rank] = s;
                    nbr[rank] = (unsigned)row;
                }
            }
            nb = nb + nnew < ef ? nb + nnew : ef;
            cur ^= 1;
        }
        __syncthreads();                                            // the new beam is whole; ctl and cand may be written again
    }

    // The first k eligible beam entries in beam order, then (-inf, -1)
    if (wave == 0) {
        i64 lab = 0, ex = -1;
        if (a.filtered) query_filter(a.filt, q, lab, ex);
        int filled = 0;
        for (int c0 = 0; c0 < nb && filled < a.k; c0 += 64) {
            const int i = c0 + lane;
            bool el = i < nb;
            i64 g = 0;
            if (el) {
                g = br[cur * ef + i] & ~GR_EXPANDED;
                if (a.filtered) {
                    const i64 gl = a.filt.mode != MI355_LABEL_ANY ? a.filt.glab[g] : 0;
                    el = eligible(a.filt.mode, lab, gl, ex, g);
                }
            }
            const unsigned long long m = __ballot(el);
            const int slot = filled + __popcll(m & ((1ull << lane) - 1ull));
            if (el && slot < a.k) {
                a.out_val[q * a.k + slot] = bs[cur * ef + i];
                a.out_idx[q * a.k + slot] = g + a.idx_offset;
            }
            filled += __popcll(m);
        }
        for (int s = (filled < a.k ? filled : a.k) + lane; s < a.k; s += 64) {
            a.out_val[q * a.k + s] = NEG_INF;
            a.out_idx[q * a.k + s] = -1;
        }
        if (lane == 0) {
            if (a.out_iters) a.out_iters[q] = iters;
            if (a.out_visited) a.out_visited[q] = visited;
        }
    }
}

// ---- host side
struct GraphWs {
    unsigned* flag; float* qn; size_t total;
};
static GraphWs graph_carve(void* ws, i64 Q, int dim) {
    GraphWs r{};
    WsCarver c(ws);
    r.flag = (unsigned*)c.take(IVF_FLAGS * sizeof(unsigned));
    r.qn = (float*)c.take((size_t)Q * dim * sizeof(float));
    r.total = c.total();
    return r;
}
// What the sizer and the entry check of the shape alike
static bool graph_shape_ok(i64 Q, int dim, int nseed, int ef, int degree, int max_iters) {
    return Q >= 1 && Q <= INT_MAX && dim >= 1 && dim <= GR_MAX_DIM && nseed >= 1 && nseed <= GR_MAX_LIST && ef >= 1 &&
           ef <= GR_MAX_EF && degree >= 2 && degree <= GR_MAX_LIST && max_iters >= 1 &&
           (i64)nseed + (i64)max_iters * degree <= GR_MAX_VISITS;
}
// The kernel asks for up to 153 KB of dynamic LDS: raise its limit once per device (as pq.hip does)
template <class Kern>
static int graph_launch(Kern kern, bool* done, dim3 grid, const GraphLds& L, hipStream_t st, const GraphArgs& a) {
    if (first_time_on_this_device(done)) {
        const GraphLds top = graph_lds(GR_MAX_DIM, GR_MAX_EF, (unsigned)(2 * GR_MAX_VISITS));
        MI355_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)top.total));
    }
    hipLaunchKernelGGL(kern, grid, dim3(GR_THREADS), L.total, st, a, L);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_graph_search_workspace_bytes(int64_t Q, int dim, int nseed, int ef, int degree, int max_iters) {
    if (!graph_shape_ok(Q, dim, nseed, ef, degree, max_iters)) return 0;
    return graph_carve(nullptr, Q, dim).total;
}

int mi355_graph_search(const float* queries, int64_t Q, int dim, float eps, const void* rows, int rows_dtype, int64_t ld, int64_t G,
                       const int32_t* graph, int degree, const int64_t* seeds, int nseed, int k, int ef, int max_iters,
                       int64_t idx_offset, const mi355_rank_filter* filter, float* out_val, int64_t* out_idx, int32_t* out_iters,
                       int32_t* out_visited, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "graph_search";
    MI355_REQUIRE(Q >= 0 && Q <= INT_MAX, "%s: Q=%lld outside [0, 2^31)", who, (long long)Q);
    MI355_REQUIRE(rows_dtype == MI355_DTYPE_F32 || rows_dtype == MI355_DTYPE_F16, "%s: unknown rows dtype %d", who, rows_dtype);
    const bool f16rows = rows_dtype == MI355_DTYPE_F16;
    MI355_REQUIRE(dim >= 1 && dim <= GR_MAX_DIM, "%s: dim=%d outside [1, %d]", who, dim, GR_MAX_DIM);
    MI355_REQUIRE(G >= 1 && G <= INT_MAX, "%s: G=%lld outside [1, 2^31)", who, (long long)G);
    MI355_REQUIRE(ld >= dim, "%s: ld=%lld < dim=%d", who, (long long)ld, dim);
    MI355_REQUIRE(k >= 1 && k <= ef && ef <= GR_MAX_EF, "%s: k=%d ef=%d outside 1 <= k <= ef <= %d", who, k, ef, GR_MAX_EF);
    MI355_REQUIRE(degree >= 2 && degree <= GR_MAX_LIST, "%s: degree=%d outside [2, %d]", who, degree, GR_MAX_LIST);
    MI355_REQUIRE(nseed >= 1 && nseed <= GR_MAX_LIST, "%s: nseed=%d outside [1, %d]", who, nseed, GR_MAX_LIST);
    MI355_REQUIRE(max_iters >= 1, "%s: max_iters=%d must be >= 1", who, max_iters);
    MI355_REQUIRE((i64)nseed + (i64)max_iters * degree <= GR_MAX_VISITS, "%s: nseed + max_iters * degree = %lld rows may be visited, "
                  "more than the %lld the visited set holds", who, (long long)nseed + (long long)max_iters * degree,
                  (long long)GR_MAX_VISITS);
    RankFilter filt{};
    if (filter)
        if (int e = make_filter(filter, idx_offset, who, &filt)) return e;
    if (Q == 0) return OK;
    MI355_REQUIRE(queries && rows && graph && seeds && out_val && out_idx, "%s: null queries/rows/graph/seeds/output pointer", who);
    MI355_REQUIRE(!f16rows || (((uintptr_t)rows & 15) == 0 && ld % 8 == 0),
                  "%s: fp16 rows must be 16-byte aligned with ld=%lld a multiple of 8", who, (long long)ld);
    const GraphWs w = graph_carve(workspace, Q, dim);
    MI355_REQUIRE(workspace && workspace_bytes >= w.total, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);

    hipStream_t st = (hipStream_t)stream;
    RoctxRange range("graph/search");
    MI355_CHECK_HIP(hipMemsetAsync(w.flag, 0, IVF_FLAGS * sizeof(unsigned), st));
    if (int e = mi355_l2_normalize_rows(queries, w.qn, Q, dim, eps, stream)) return e;

    GraphArgs a{};
    a.qn = w.qn; a.rows = rows; a.ld = ld; a.G = G; a.dim = dim; a.ldq = row_dot_ldq(dim, f16rows);
    a.graph = graph; a.seeds = (const i64*)seeds; a.degree = degree; a.nseed = nseed; a.k = k; a.ef = ef; a.max_iters = max_iters;
    a.tsize = graph_table_slots(nseed, max_iters, degree);
    a.idx_offset = idx_offset; a.out_val = out_val; a.out_idx = (i64*)out_idx; a.out_iters = out_iters; a.out_visited = out_visited;
    a.flag = w.flag; a.filt = filt; a.filtered = filter != nullptr;
    const GraphLds L = graph_lds(a.ldq, ef, a.tsize);
    const dim3 grid((unsigned)Q);
    static bool done[3][MI355_MAX_DEVICES] = {{false}};
    int e;
    if (f16rows) e = graph_launch(k_graph_search<true, true>, done[0], grid, L, st, a);
    else if (ld % 4 == 0 && dim % 4 == 0 && ((uintptr_t)rows & 15) == 0) e = graph_launch(k_graph_search<false, true>, done[1], grid, L, st, a);
    else e = graph_launch(k_graph_search<false, false>, done[2], grid, L, st, a);
    if (e) return e;

    // the one read of the flag, behind the launch (ivf.hip's scheme)
    unsigned flags[IVF_FLAGS] = {0, 0};
    MI355_CHECK_HIP(hipMemcpyAsync(flags, w.flag, sizeof(flags), hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    MI355_REQUIRE(!flags[IVF_FLAG_ENTRY], "%s: a seed or a graph entry outside [0, G=%lld) other than -1", who, (long long)G);
    return OK;
}

}  // extern "C"
