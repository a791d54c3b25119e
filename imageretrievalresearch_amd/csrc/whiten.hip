// PCA whitening of embeddings: the float64 moments of the fit (mi355_embedding_moments) and the fused transform
// normalise -> project -> bias -> normalise (mi355_whiten_rows).  gfx950 only.  Semantics: include/mi355_retrieval.h.
//
// Moments.  outer[i][j] = sum_r x[r][i] * x[r][j] is a GEMM whose reduction axis is the rows.  The (i, j) plane is cut into
// 128 x 128 tiles and only tiles with ti <= tj are computed; a 256-thread workgroup owns one tile over one SPLIT of the rows,
// each of its four waves a 64 x 64 quarter as 4 x 4 v_mfma_f64_16x16x4_f64 accumulators (128 VGPRs).  Rows go through LDS
// 16 at a time as fp32 (fp16 rows widened, normalised rows scaled with the library's 1 / norm) and are widened to f64 when a
// lane reads its operand: fp32 -> f64 is exact and so is the f64 product of two of them, the only rounding is the f64
// accumulation.  The A and B operands have the same lane map (row of the chunk = lane >> 4, column = lane & 15), rows of the
// LDS image are 144 floats apart so that the four rows a wave reads fall into different banks.
// Determinism: the number of splits and the rows of each are a function of (R, dim) alone (moments_plan: about 1024
// workgroups, two rounds of two workgroups per CU of this chip, never read from the device).  Every (split, tile) writes its
// partial tile to the workspace; a second kernel adds the partials in split order, adds the caller's value (accumulate) and
// writes the element and its mirror.  No floating-point atomics anywhere.  The row sums ride along in the diagonal tiles:
// thread (column, row parity) adds its staged values in row order, the two parities are combined in a fixed order.
//
// Transform.  One workgroup owns 64 rows and walks the output columns 128 at a time; a wave owns 32 rows x 64 columns as two
// v_mfma_f32_32x32x2_f32 accumulators that start from the bias.  That MFMA is bit for bit an fp32 fmaf chain, so y[j] is
// fma(m[j][i], x[i], ...) over i in one fixed order (per 8 inputs: 0, 4, 1, 5, 2, 6, 3, 7) whatever R is and wherever the row
// sits in its tile.  The un-normalised y goes to the output rows (fp32) or to workspace rows (fp16 output); after a barrier
// each wave finishes rows with normalize_row_store, the device code mi355_expand_rows ends with: the library's norm with its
// summation order, then scale (fp32) or scale and round with zeroed pads (fp16).
#include "rank_common.h"
#include "../../include/mi355_retrieval.h"

#include <math.h>

namespace mi355 {

typedef _Float16 f16;
typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float pinned_f32(float p) {
    asm volatile("" : "+v"(p));          // no instruction: keeps p a rounded fp32 value
    return p;
}

static bool rows_aligned(const void* p, i64 ld, int elem, int align) {
    return ((uintptr_t)p % align) == 0 && (ld * elem) % align == 0;
}

// 1 / norm of each row as mi355_l2_normalize_rows takes it (one wave per row)
__global__ __launch_bounds__(256) void k_rows_inv_norm(const float* __restrict__ in, i64 ld, float* __restrict__ inv, i64 rows,
                                                       int dim, float eps, int vec) {
    const int lane = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float r = row_inv_norm(in + row * ld, dim, eps, vec, lane);
    if (lane == 0) inv[row] = r;
}

// =====================================================================================
// moments
// =====================================================================================
constexpr int MO_BT = 128;                 // tile edge
constexpr int MO_KC = 16;                  // rows per LDS chunk
constexpr int MO_LD = MO_BT + 16;          // floats between rows of the LDS image
constexpr int MO_WGS = 1024;               // workgroups a call aims at (fixed: the split must not depend on the device)
constexpr int MO_MIN_ROWS = 128;           // a split has at least this many rows
constexpr int MO_MAX_DIM = 16384;

struct MomentsPlan {
    int T;              // tiles per axis
    int ntiles;         // T (T + 1) / 2
    int S;              // splits of the rows
    i64 chunk;          // rows per split (a multiple of MO_KC)
    size_t off_part, off_sum, total;     // workspace: [R] 1 / norm, [S][ntiles][128][128] partial tiles, [S][T][128] partial sums
};

static MomentsPlan moments_plan(i64 R, int dim) {
    MomentsPlan p{};
    p.T = (dim + MO_BT - 1) / MO_BT;
    p.ntiles = p.T * (p.T + 1) / 2;
    i64 s = MO_WGS / p.ntiles;
    const i64 smax = (R + MO_MIN_ROWS - 1) / MO_MIN_ROWS;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const i64 per = (R + s - 1) / s;
    p.chunk = (per + MO_KC - 1) / MO_KC * MO_KC;
    if (p.chunk < MO_KC) p.chunk = MO_KC;
    p.S = (int)((R + p.chunk - 1) / p.chunk);
    if (p.S < 1) p.S = 1;
    p.off_part = align_up((size_t)(R > 0 ? R : 0) * sizeof(float), 256);
    p.off_sum = p.off_part + (size_t)p.S * p.ntiles * MO_BT * MO_BT * sizeof(double);
    p.total = p.off_sum + (size_t)p.S * p.T * MO_BT * sizeof(double);
    return p;
}

// tile t of the upper triangle, row-major: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void moments_tile_of(int t, int T, int& ti, int& tj) {
    ti = 0;
    while (t >= T - ti) { t -= T - ti; ++ti; }
    tj = ti + t;
}

template <class TI, bool NORM>
__global__ __launch_bounds__(256, 2) void k_moments(const TI* __restrict__ rows, i64 R, i64 ld, int dim,
                                                    const float* __restrict__ rinv, i64 chunk, int T, int ntiles,
                                                    double* __restrict__ part, double* __restrict__ psum) {
    __shared__ float As[MO_KC * MO_LD];
    __shared__ float Bs[MO_KC * MO_LD];
    __shared__ double csum[MO_BT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int t = blockIdx.x, s = blockIdx.y;
    int ti, tj;
    moments_tile_of(t, T, ti, tj);
    const bool diag = ti == tj;
    const int i0 = ti * MO_BT, j0 = tj * MO_BT;
    const i64 r_begin = (i64)s * chunk;
    const i64 r_end = r_begin + chunk < R ? r_begin + chunk : R;
    // this wave's 64 x 64 quarter: nothing of it is used below the diagonal of a diagonal tile or past dim
    const bool work = !(diag && wm > wn) && i0 + wm * 64 < dim && j0 + wn * 64 < dim;

    f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double cs = 0.0;

    const int c = tid & 127, rh = tid >> 7;          // staging: column c of the tile, rows rh, rh + 2, ..
    const bool ca = i0 + c < dim, cb = j0 + c < dim;
    float ra[MO_KC / 2], rb[MO_KC / 2];
    auto fetch = [&](i64 r, int col) -> float {
        float v = (float)rows[r * ld + col];
        if constexpr (NORM) v = pinned_f32(v * rinv[r]);
        return v;
    };
    auto load = [&](i64 r0) {
#pragma unroll
        for (int e = 0; e < MO_KC / 2; ++e) {
            const i64 r = r0 + rh + 2 * e;
            const bool in = r < r_end;
            ra[e] = in && ca ? fetch(r, i0 + c) : 0.f;
            rb[e] = diag ? ra[e] : (in && cb ? fetch(r, j0 + c) : 0.f);
        }
    };

    if (r_begin < r_end) load(r_begin);
    for (i64 r0 = r_begin; r0 < r_end; r0 += MO_KC) {
#pragma unroll
        for (int e = 0; e < MO_KC / 2; ++e) {
            As[(rh + 2 * e) * MO_LD + c] = ra[e];
            Bs[(rh + 2 * e) * MO_LD + c] = rb[e];
            if (diag) cs += (double)ra[e];
        }
        __syncthreads();
        if (r0 + MO_KC < r_end) load(r0 + MO_KC);
        if (work) {
            const float* a = As + (lane >> 4) * MO_LD + wm * 64 + (lane & 15);
            const float* b = Bs + (lane >> 4) * MO_LD + wn * 64 + (lane & 15);
#pragma unroll
            for (int kk = 0; kk < MO_KC / 4; ++kk) {
                double av[4], bv[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    av[m] = (double)a[kk * 4 * MO_LD + m * 16];
                    bv[m] = (double)b[kk * 4 * MO_LD + m * 16];
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[n], acc[m][n], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg
    if (work) {
        double* p = part + ((size_t)s * ntiles + t) * (MO_BT * MO_BT);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = wm * 64 + m * 16 + (lane >> 4) + 4 * reg, col = wn * 64 + n * 16 + (lane & 15);
                    p[row * MO_BT + col] = acc[m][n][reg];
                }
    }
    if (diag) {
        if (rh == 1) csum[c] = cs;
        __syncthreads();
        if (rh == 0) psum[((size_t)s * T + ti) * MO_BT + c] = cs + csum[c];
    }
}

// Partials -> sum / outer in split order; the element and its mirror get the same bits.  grid (ntiles, 64)
__global__ __launch_bounds__(256) void k_moments_reduce(const double* __restrict__ part, const double* __restrict__ psum, int S,
                                                        int T, int ntiles, int dim, int accumulate, double* __restrict__ sum,
                                                        double* __restrict__ outer) {
    const int t = blockIdx.x;
    int ti, tj;
    moments_tile_of(t, T, ti, tj);
    const int e = blockIdx.y * 256 + threadIdx.x, row = e >> 7, col = e & 127;
    const int i = ti * MO_BT + row, j = tj * MO_BT + col;
    if (i < dim && j < dim && i <= j) {
        double v = 0.0;
        for (int s = 0; s < S; ++s) v += part[((size_t)s * ntiles + t) * (MO_BT * MO_BT) + e];
        if (accumulate) v = outer[(size_t)i * dim + j] + v;
        outer[(size_t)i * dim + j] = v;
        outer[(size_t)j * dim + i] = v;
    }
    if (ti == tj && blockIdx.y == 0 && threadIdx.x < MO_BT && ti * MO_BT + (int)threadIdx.x < dim) {
        const int q = ti * MO_BT + threadIdx.x;
        double v = 0.0;
        for (int s = 0; s < S; ++s) v += psum[((size_t)s * T + ti) * MO_BT + threadIdx.x];
        sum[q] = accumulate ? sum[q] + v : v;
    }
}

// =====================================================================================
// transform
// =====================================================================================
constexpr int WH_BM = 64, WH_BN = 128, WH_BK = 32, WH_LD = WH_BK + 4;

struct WhitenArgs {
    const void* x; i64 R, x_ld; int x_f16, norm_in, x_vec;
    float eps;
    const float* mat; const float* bias;
    int din, dout;
    float* y; i64 y_ld;        // the un-normalised rows: the output rows (fp32) or workspace rows (fp16 output)
    void* out; i64 out_ld;
};

template <bool VEC, bool OF16, bool NORM_OUT>
__global__ __launch_bounds__(256, 2) void k_whiten_rows(WhitenArgs a) {
    __shared__ float Xs[WH_BM * WH_LD];
    __shared__ float Ms[WH_BN * WH_LD];
    __shared__ float rin[WH_BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lk = (lane >> 5) * 4;
    const i64 m0 = (i64)blockIdx.x * WH_BM;
    const float* xf = a.x_f16 ? nullptr : static_cast<const float*>(a.x);
    const f16* xh = a.x_f16 ? static_cast<const f16*>(a.x) : nullptr;
    const int din = a.din, dout = a.dout;

    if (a.norm_in) {
        for (int rr = wave; rr < WH_BM; rr += 4) {
            const i64 row = m0 + rr;
            const float r = row < a.R ? row_inv_norm(xf + row * a.x_ld, din, a.eps, a.x_vec, lane) : 0.f;
            if (lane == 0) rin[rr] = r;
        }
        __syncthreads();
    }

    const int kx = tid & 31, r8 = tid >> 5;
    for (int n0 = 0; n0 < dout; n0 += WH_BN) {
        const bool work = n0 + wn * 64 < dout;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + j * 32 + lr;
            const float b = col < dout ? a.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = b;
        }
        for (int k0 = 0; k0 < din; k0 += WH_BK) {
            const bool kin = k0 + kx < din;
#pragma unroll
            for (int e = 0; e < WH_BM / 8; ++e) {
                const int rr = r8 + 8 * e;
                const i64 row = m0 + rr;
                float v = 0.f;
                if (kin && row < a.R) {
                    v = a.x_f16 ? (float)xh[row * a.x_ld + k0 + kx] : xf[row * a.x_ld + k0 + kx];
                    if (a.norm_in) v = pinned_f32(v * rin[rr]);
                }
                Xs[rr * WH_LD + kx] = v;
            }
#pragma unroll
            for (int e = 0; e < WH_BN / 8; ++e) {
                const int cc = r8 + 8 * e;
                Ms[cc * WH_LD + kx] = (kin && n0 + cc < dout) ? a.mat[(size_t)(n0 + cc) * din + k0 + kx] : 0.f;
            }
            __syncthreads();
            if (work) {
                const float* xa = Xs + (wm * 32 + lr) * WH_LD + lk;
                const float* mb = Ms + (wn * 64 + lr) * WH_LD + lk;
#pragma unroll
                for (int t8 = 0; t8 < WH_BK / 8; ++t8) {
                    const f32x4 af = *reinterpret_cast<const f32x4*>(xa + t8 * 8);
                    f32x4 bf[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const f32x4*>(mb + j * 32 * WH_LD + t8 * 8);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[j][e], acc[j], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // C[row][col]: lane: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + j * 32 + lr;
            if (col >= dout) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const i64 row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < a.R) a.y[row * a.y_ld + col] = acc[j][r];
            }
        }
    }
    if constexpr (NORM_OUT) {
        __threadfence_block();
        __syncthreads();                              // every y of the 64 rows is written and visible to the workgroup
        for (int rr = wave; rr < WH_BM; rr += 4) {
            const i64 row = m0 + rr;
            if (row >= a.R) break;
            f16* h = OF16 ? static_cast<f16*>(a.out) + row * a.out_ld : nullptr;
            normalize_row_store<VEC, OF16>(a.y + row * a.y_ld, h, dout, (int)a.out_ld, a.eps, lane);
        }
    }
}

template <bool VEC>
static void launch_whiten(const WhitenArgs& a, int out_f16, int norm_out, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(a.R, WH_BM));
    if (out_f16) hipLaunchKernelGGL((k_whiten_rows<VEC, true, true>), grid, dim3(256), 0, st, a);
    else if (norm_out) hipLaunchKernelGGL((k_whiten_rows<VEC, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_whiten_rows<VEC, false, false>), grid, dim3(256), 0, st, a);
}

}  // namespace mi355

using namespace mi355;

extern "C" {

size_t mi355_moments_workspace_bytes(int64_t R, int dim) {
    if (R < 1 || dim < 1 || dim > MO_MAX_DIM) return 0;
    return moments_plan(R, dim).total;
}

int mi355_embedding_moments(const void* rows, int rows_dtype, int64_t R, int64_t ld, int dim, int normalize_rows, float eps,
                            int accumulate, double* sum, double* outer, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "embedding_moments";
    MI355_REQUIRE(sum && outer && (rows || R == 0), "%s: null pointer", who);
    MI355_REQUIRE(rows_dtype == MI355_DTYPE_F32 || rows_dtype == MI355_DTYPE_F16,
                  "%s: dtype %d is neither MI355_DTYPE_F32 nor MI355_DTYPE_F16", who, rows_dtype);
    MI355_REQUIRE(dim >= 1 && dim <= MO_MAX_DIM && R >= 0 && R <= ((int64_t)1 << 40), "%s: bad shape R=%lld dim=%d (dim in [1, %d])",
                  who, (long long)R, dim, MO_MAX_DIM);
    MI355_REQUIRE(ld >= dim, "%s: leading dim ld=%lld must be >= dim=%d", who, (long long)ld, dim);
    MI355_REQUIRE(!normalize_rows || rows_dtype == MI355_DTYPE_F32, "%s: normalize_rows needs fp32 rows", who);
    MI355_REQUIRE(isfinite(eps) && eps >= 0.f, "%s: eps must be finite and >= 0, got %g", who, (double)eps);
    const size_t need = mi355_moments_workspace_bytes(R, dim);
    MI355_REQUIRE(!need || (workspace && ((uintptr_t)workspace & 15) == 0), "%s: needs a 16-byte aligned workspace", who);
    MI355_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    if (R == 0) {
        if (!accumulate) {
            MI355_CHECK_HIP(hipMemsetAsync(sum, 0, (size_t)dim * sizeof(double), st));
            MI355_CHECK_HIP(hipMemsetAsync(outer, 0, (size_t)dim * dim * sizeof(double), st));
        }
        return OK;
    }
    const MomentsPlan p = moments_plan(R, dim);
    float* rinv = (float*)workspace;
    double* part = (double*)((char*)workspace + p.off_part);
    double* psum = (double*)((char*)workspace + p.off_sum);
    if (normalize_rows) {
        const int vec = dim % 4 == 0 && rows_aligned(rows, ld, 4, 16);
        hipLaunchKernelGGL(k_rows_inv_norm, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, st, (const float*)rows, (i64)ld, rinv, (i64)R,
                           dim, eps, vec);
        MI355_LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)p.ntiles, (unsigned)p.S);
    if (rows_dtype == MI355_DTYPE_F16)
        hipLaunchKernelGGL((k_moments<f16, false>), grid, dim3(256), 0, st, (const f16*)rows, (i64)R, (i64)ld, dim,
                           (const float*)nullptr, p.chunk, p.T, p.ntiles, part, psum);
    else if (normalize_rows)
        hipLaunchKernelGGL((k_moments<float, true>), grid, dim3(256), 0, st, (const float*)rows, (i64)R, (i64)ld, dim,
                           (const float*)rinv, p.chunk, p.T, p.ntiles, part, psum);
    else
        hipLaunchKernelGGL((k_moments<float, false>), grid, dim3(256), 0, st, (const float*)rows, (i64)R, (i64)ld, dim,
                           (const float*)nullptr, p.chunk, p.T, p.ntiles, part, psum);
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_moments_reduce, dim3((unsigned)p.ntiles, MO_BT * MO_BT / 256), dim3(256), 0, st, (const double*)part,
                       (const double*)psum, p.S, p.T, p.ntiles, dim, accumulate ? 1 : 0, sum, outer);
    MI355_LAUNCH_CHECK();
    return OK;
}

size_t mi355_whiten_workspace_bytes(int64_t R, int dim_in, int dim_out, int out_dtype) {
    if (R < 1 || dim_in < 1 || dim_out < 1 || out_dtype != MI355_DTYPE_F16) return 0;
    return (size_t)R * (size_t)dim_out * sizeof(float);
}

int mi355_whiten_rows(const void* x, int x_dtype, int64_t R, int64_t x_ld, int dim_in, int normalize_input, float eps,
                      const float* matrix, const float* bias, int dim_out, int normalize_output, void* out, int out_dtype,
                      int64_t out_ld, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "whiten_rows";
    MI355_REQUIRE(x && matrix && bias && out, "%s: null pointer", who);
    for (int d : {x_dtype, out_dtype})
        MI355_REQUIRE(d == MI355_DTYPE_F32 || d == MI355_DTYPE_F16, "%s: dtype %d is neither MI355_DTYPE_F32 nor MI355_DTYPE_F16",
                      who, d);
    MI355_REQUIRE(dim_in >= 1 && R >= 0 && R <= ((int64_t)1 << 36), "%s: bad shape R=%lld dim_in=%d", who, (long long)R, dim_in);
    MI355_REQUIRE(dim_out >= 1 && dim_out <= dim_in, "%s: dim_out=%d outside [1, dim_in=%d]", who, dim_out, dim_in);
    MI355_REQUIRE(x_ld >= dim_in && out_ld >= dim_out && out_ld <= INT_MAX,
                  "%s: leading dims must be >= the row length (x_ld=%lld dim_in=%d out_ld=%lld dim_out=%d)", who, (long long)x_ld,
                  dim_in, (long long)out_ld, dim_out);
    MI355_REQUIRE(!normalize_input || x_dtype == MI355_DTYPE_F32, "%s: normalize_input needs fp32 rows", who);
    const bool of16 = out_dtype == MI355_DTYPE_F16;
    MI355_REQUIRE(!of16 || normalize_output, "%s: fp16 output stores normalised rows (normalize_output)", who);
    MI355_REQUIRE(isfinite(eps) && eps >= 0.f, "%s: eps must be finite and >= 0, got %g", who, (double)eps);
    const bool vec = dim_out % 4 == 0;
    MI355_REQUIRE(!vec || !normalize_output || (((uintptr_t)out & 15) == 0 && out_ld % 4 == 0),
                  "%s: with dim_out %% 4 == 0 the output must be 16-byte aligned and out_ld=%lld a multiple of 4", who,
                  (long long)out_ld);
    if (of16) {
        const size_t need = mi355_whiten_workspace_bytes(R, dim_in, dim_out, out_dtype);
        MI355_REQUIRE(!need || (workspace && ((uintptr_t)workspace & 15) == 0), "%s: fp16 output needs a 16-byte aligned workspace",
                      who);
        MI355_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    }
    if (R == 0) return OK;
    WhitenArgs a{};
    a.x = x; a.R = R; a.x_ld = x_ld; a.x_f16 = x_dtype == MI355_DTYPE_F16; a.norm_in = normalize_input ? 1 : 0;
    // the input's own norm: the vec rule of mi355_l2_normalize_rows
    a.x_vec = !a.x_f16 && dim_in % 4 == 0 && rows_aligned(x, x_ld, 4, 16);
    a.eps = eps; a.mat = matrix; a.bias = bias; a.din = dim_in; a.dout = dim_out;
    a.y = of16 ? (float*)workspace : (float*)out;
    a.y_ld = of16 ? dim_out : out_ld;
    a.out = out; a.out_ld = out_ld;
    hipStream_t st = (hipStream_t)stream;
    if (vec) launch_whiten<true>(a, of16, normalize_output, st);
    else launch_whiten<false>(a, of16, normalize_output, st);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
