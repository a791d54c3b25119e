// Query expansion (alpha-QE) and database-side augmentation (DBA): mi355_expand_rows.  gfx950 only.
//
// Output row r (include/mi355_retrieval.h):
//   x   = base_r + sum_{j < n, slot j used} w_j * row(i_j - idx_offset)      fp32, per element, j in rank order
//   w_j = v_j ^ alpha, a slot is used iff v_j > 0 and i_j - idx_offset is a row of the gallery (else skipped, never read)
//   out = l2_normalize_rows(x) bit for bit (fp32), or its fp16 rounding as mi355_gallery_to_f16 stores it (fp16)
// base_r is the base row as it is, or l2_normalize_rows(base_r) (normalize_base).
//
// One wave per output row, four rows per 256-thread workgroup (the layout of k_row_norm / k_rows_to_f16).  A lane owns the
// chunks of the row that row_inv_norm gives it (float4 i = lane + 64 t when vec, element i = lane + 64 t otherwise), keeps
// their fp32 sums in registers, PC units per pass, and gathers the neighbour rows four at a time (wave-uniform index and
// weight, read once per 64 slots into lanes and broadcast with readlane).  The sum x is stored in that same mapping - into
// the output row (fp32) or a workspace row (fp16) - and row_inv_norm reads it back: every lane reads only what it wrote,
// so no barrier is needed, and the norm is the library's one function with its summation order.  Then scale and store.
// Each product w_j * row and the normalised base are pinned in a register before the add, so -ffp-contract=fast cannot
// fuse them into an fma: the sum has the roundings of `x = x + w * row` done one operation at a time.
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <math.h>

namespace mi355 {

typedef _Float16 f16;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// w = v ^ alpha: alpha 0, 1, 2, 3 as 1, v, v * v, (v * v) * v (torch's own special cases of `v ** alpha`), else powf
__device__ __forceinline__ float qe_weight(float v, float alpha) {
    if (alpha == 0.f) return 1.f;
    if (alpha == 1.f) return v;
    if (alpha == 2.f) return v * v;
    if (alpha == 3.f) {
        const float s = v * v;
        return s * v;
    }
    return powf(v, alpha);
}

__device__ __forceinline__ float pinned(float p) {
    asm volatile("" : "+v"(p));          // no instruction: keeps p a rounded fp32 value (no fma across it)
    return p;
}

// Unit u of a row (W = 4: float4 chunk u, W = 1: element u) widened to fp32; v4: the row is aligned for one vector load
template <int W>
__device__ __forceinline__ void load_unit(const float* row, i64 u, int v4, float (&o)[W]) {
    if constexpr (W == 4) {
        if (v4) {
            const f32x4 v = reinterpret_cast<const f32x4*>(row)[u];
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = row[u * W + e];
}
template <int W>
__device__ __forceinline__ void load_unit(const f16* row, i64 u, int v4, float (&o)[W]) {
    if constexpr (W == 4) {
        if (v4) {
            const f16x4 h = reinterpret_cast<const f16x4*>(row)[u];
            o[0] = (float)h.x; o[1] = (float)h.y; o[2] = (float)h.z; o[3] = (float)h.w;
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = (float)row[u * W + e];
}

struct ExpandArgs {
    const void* base; i64 base_ld; int base_f16; int normalize_base; int base_vec; int base_v4;
    const void* gal; i64 G; i64 gld; int gal_v4;
    const float* vals; const i64* idx; i64 R; int n; i64 idx_offset;
    float alpha, eps;
    void* out; i64 out_ld;
    float* xws;            // fp16 output: [R][dim] fp32 sums; null for fp32 output (the sum goes to the output row)
    int dim;
};

template <bool VEC, class TG, bool OF16>
__global__ __launch_bounds__(256, 4) void k_expand_rows(ExpandArgs a) {
    constexpr int W = VEC ? 4 : 1;             // elements per unit
    constexpr int PC = VEC ? 4 : 16;           // units per lane and pass (16 fp32 accumulators)
    constexpr int NB = 4;                      // neighbour rows in flight
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.R) return;
    const int dim = a.dim, nu = dim / W;
    const TG* gal = static_cast<const TG*>(a.gal);
    float* x = OF16 ? a.xws + row * dim : static_cast<float*>(a.out) + row * a.out_ld;
    const float* bf = a.base_f16 ? nullptr : static_cast<const float*>(a.base) + row * a.base_ld;
    const f16* bh = a.base_f16 ? static_cast<const f16*>(a.base) + row * a.base_ld : nullptr;
    const float rb = a.normalize_base ? row_inv_norm(bf, dim, a.eps, a.base_vec, lane) : 1.0f;
    const float* vrow = a.vals + row * a.n;
    const i64* irow = a.idx + row * a.n;

    for (int u0 = 0; u0 < nu; u0 += 64 * PC) {
        float acc[PC][W];
#pragma unroll
        for (int p = 0; p < PC; ++p) {
            const i64 u = u0 + lane + 64 * p;
            for (int e = 0; e < W; ++e) acc[p][e] = 0.f;
            if (u < nu) {
                if (a.base_f16) load_unit<W>(bh, u, a.base_v4, acc[p]);
                else load_unit<W>(bf, u, a.base_v4, acc[p]);
                if (a.normalize_base) {
#pragma unroll
                    for (int e = 0; e < W; ++e) acc[p][e] = pinned(acc[p][e] * rb);
                }
            }
        }
        for (int s0 = 0; s0 < a.n; s0 += 64) {
            // this lane's slot s0 + lane: its weight and local row (-1: skipped)
            float wl = 0.f;
            i64 ll = -1;
            if (s0 + lane < a.n) {
                const float v = vrow[s0 + lane];
                const i64 l = irow[s0 + lane] - a.idx_offset;
                if (v > 0.f && l >= 0 && l < a.G) {
                    wl = qe_weight(v, a.alpha);
                    ll = l;
                }
            }
            const int lo = (int)(ll & 0xffffffff), hi = (int)(ll >> 32);
            const int m = a.n - s0 < 64 ? a.n - s0 : 64;
            for (int j0 = 0; j0 < m; j0 += NB) {
                float nbv[NB][PC][W];
                float wj[NB];
                i64 lj[NB];
#pragma unroll
                for (int t = 0; t < NB; ++t) {               // wave-uniform: scalar registers, uniform branches
                    const int j = j0 + t < m ? j0 + t : m - 1;
                    wj[t] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), j));
                    lj[t] = j0 + t < m ? (i64)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, j) << 32) |
                                              (unsigned)__builtin_amdgcn_readlane(lo, j))
                                       : -1;
                }
#pragma unroll
                for (int t = 0; t < NB; ++t) {               // issue every load of the group first
                    if (lj[t] >= 0) {
                        const TG* g = gal + lj[t] * a.gld;
#pragma unroll
                        for (int p = 0; p < PC; ++p) {
                            const i64 u = u0 + lane + 64 * p;
                            if (u < nu) load_unit<W>(g, u, a.gal_v4, nbv[t][p]);
                            else
                                for (int e = 0; e < W; ++e) nbv[t][p][e] = 0.f;
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < NB; ++t) {               // then add in rank order
                    if (lj[t] >= 0) {
#pragma unroll
                        for (int p = 0; p < PC; ++p)
#pragma unroll
                            for (int e = 0; e < W; ++e) acc[p][e] += pinned(wj[t] * nbv[t][p][e]);
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PC; ++p) {
            const i64 u = u0 + lane + 64 * p;
            if (u < nu) {
                if constexpr (VEC) reinterpret_cast<f32x4*>(x)[u] = (f32x4){acc[p][0], acc[p][1], acc[p][2], acc[p][3]};
                else x[u] = acc[p][0];
            }
        }
    }
    // the norm of x as l2_normalize_rows takes it (each lane reads back only its own units), then scale and store
    f16* y = OF16 ? static_cast<f16*>(a.out) + row * a.out_ld : nullptr;
    normalize_row_store<VEC, OF16>(x, y, dim, (int)a.out_ld, a.eps, lane);
}

template <bool VEC, class TG>
static void launch_expand(const ExpandArgs& a, int out_f16, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(a.R, 4));
    if (out_f16) hipLaunchKernelGGL((k_expand_rows<VEC, TG, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_expand_rows<VEC, TG, false>), grid, dim3(256), 0, st, a);
}

static bool aligned_rows(const void* p, i64 ld, int elem, int align) {
    return ((uintptr_t)p % align) == 0 && (ld * elem) % align == 0;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_expand_workspace_bytes(int64_t R, int dim, int out_dtype) {
    if (R < 1 || dim < 1 || out_dtype != MI355_DTYPE_F16) return 0;
    return (size_t)R * (size_t)dim * sizeof(float);
}

int mi355_expand_rows(const void* base, int base_dtype, int64_t base_ld, int normalize_base, const void* gallery,
                      int gallery_dtype, int64_t gallery_rows, int64_t gallery_ld, int dim, const float* vals,
                      const int64_t* idx, int64_t R, int n, int64_t idx_offset, float alpha, float eps, void* out,
                      int out_dtype, int64_t out_ld, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "expand_rows";
    MI355_REQUIRE(base && gallery && vals && idx && out, "%s: null pointer", who);
    for (int d : {base_dtype, gallery_dtype, out_dtype})
        MI355_REQUIRE(d == MI355_DTYPE_F32 || d == MI355_DTYPE_F16, "%s: dtype %d is neither MI355_DTYPE_F32 nor MI355_DTYPE_F16",
                      who, d);
    MI355_REQUIRE(dim >= 1 && R >= 0 && gallery_rows >= 0, "%s: bad shape R=%lld gallery_rows=%lld dim=%d", who, (long long)R,
                  (long long)gallery_rows, dim);
    MI355_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n=%d outside [1, 2^20]", who, n);
    MI355_REQUIRE(isfinite(alpha) && alpha >= 0.f, "%s: alpha must be finite and >= 0, got %g", who, (double)alpha);
    MI355_REQUIRE(isfinite(eps) && eps >= 0.f, "%s: eps must be finite and >= 0, got %g", who, (double)eps);
    MI355_REQUIRE(base_ld >= dim && gallery_ld >= dim && out_ld >= dim,
                  "%s: leading dims must be >= dim=%d (base_ld=%lld gallery_ld=%lld out_ld=%lld)", who, dim, (long long)base_ld,
                  (long long)gallery_ld, (long long)out_ld);
    MI355_REQUIRE(!normalize_base || base_dtype == MI355_DTYPE_F32, "%s: normalize_base needs fp32 base rows", who);
    MI355_REQUIRE(R <= ((int64_t)1 << 40) && gallery_rows <= ((int64_t)1 << 40) && out_ld <= INT_MAX,
                  "%s: shape too large R=%lld gallery_rows=%lld", who, (long long)R, (long long)gallery_rows);
    const bool vec = dim % 4 == 0;
    MI355_REQUIRE(!vec || (((uintptr_t)out & 15) == 0 && out_ld % 4 == 0),
                  "%s: with dim %% 4 == 0 the output must be 16-byte aligned and out_ld=%lld a multiple of 4", who,
                  (long long)out_ld);
    const bool of16 = out_dtype == MI355_DTYPE_F16;
    if (of16) {
        const size_t need = mi355_expand_workspace_bytes(R, dim, out_dtype);
        MI355_REQUIRE(!need || (workspace && ((uintptr_t)workspace & 15) == 0),
                      "%s: fp16 output needs a 16-byte aligned workspace", who);
        MI355_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    }
    if (R == 0) return OK;
    ExpandArgs a{};
    a.base = base; a.base_ld = base_ld; a.base_f16 = base_dtype == MI355_DTYPE_F16; a.normalize_base = normalize_base ? 1 : 0;
    // the base's own norm: the vec rule of mi355_l2_normalize_rows (into a fresh, aligned output)
    a.base_vec = !a.base_f16 && vec && aligned_rows(base, base_ld, 4, 16);
    a.base_v4 = vec && aligned_rows(base, base_ld, a.base_f16 ? 2 : 4, a.base_f16 ? 8 : 16);
    const bool gf16 = gallery_dtype == MI355_DTYPE_F16;
    a.gal = gallery; a.G = gallery_rows; a.gld = gallery_ld;
    a.gal_v4 = vec && aligned_rows(gallery, gallery_ld, gf16 ? 2 : 4, gf16 ? 8 : 16);
    a.vals = vals; a.idx = (const i64*)idx; a.R = R; a.n = n; a.idx_offset = idx_offset;
    a.alpha = alpha; a.eps = eps;
    a.out = out; a.out_ld = out_ld; a.xws = of16 ? (float*)workspace : nullptr;
    a.dim = dim;
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        if (gf16) launch_expand<true, f16>(a, of16, st);
        else launch_expand<true, float>(a, of16, st);
    } else {
        if (gf16) launch_expand<false, f16>(a, of16, st);
        else launch_expand<false, float>(a, of16, st);
    }
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
