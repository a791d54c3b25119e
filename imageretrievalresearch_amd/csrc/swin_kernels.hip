// Swin kernels: patch embed (+LN), LayerNorm (plain / 2x2 patch-merge gather / final LN + token mean) and the
// MFMA window-attention kernel with fused relative-position bias, shift mask and softmax.  gfx950 only.
//
// Attention maps one wave to one (image, window, head): 49 tokens x head_dim 32.  S^T = K Q^T runs on
// mfma_f32_16x16x32_bf16 with BOTH operands loaded straight from the qkv tensor in fragment layout (a lane needs
// 16 contiguous bytes of one token row); with keys on the MFMA rows a lane ends up with 16 keys of ONE query, so
// the softmax reduction is in-lane + two xor-shuffles, and the probabilities are already in B-operand layout for
// O^T = V^T P^T (k permuted the same way on the V^T side).  Only V goes through LDS (transposed, 4.6 KB / wave).
#include "model_exec.h"
#include "../../include/mi355_retrieval.h"

#include <algorithm>
#include <vector>
#include <type_traits>

namespace mi355 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void sw_unpack8(u32x4 v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ u32x4 sw_pack8(const float* f) {
    u32x4 o;
    o.x = pack2bf(f[0], f[1]); o.y = pack2bf(f[2], f[3]); o.z = pack2bf(f[4], f[5]); o.w = pack2bf(f[6], f[7]);
    return o;
}
template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// =====================================================================================
// patch embed: conv 4x4 stride 4 (3 -> 128) + bias, then LayerNorm(128).
// w [48][128] fp32 (k = ci*16 + dy*4 + dx), values pre-rounded to bf16.
// Block = two rows of patches (PE_P = 2*gw <= 128 patches): the 24 image rows they cover are read as whole float4s
// into LDS; thread = (channel group of 8, patch group) and keeps PE_PPT patches in registers, so each weight vector it
// loads feeds PE_PPT*8 FMAs (the first version, one patch per thread, issued 96 weight loads per 8 outputs and was
// bound by the texture-address unit: 0.32 ms for B = 128).
// =====================================================================================
constexpr int PE_PPT = 7;          // patches per thread
constexpr int PE_PG = 16;          // patch groups per block (x 16 channel groups = 256 threads)
constexpr int PE_P = PE_PPT * PE_PG;   // 112 patches per block = 2 patch rows at gw = 56
// U8: the input is a batch of decoded uint8 images [B][h][w][3] and the reference's inference transform - SquarePad(fill) ->
// ToTensor -> Normalize(mean, std), inference/inference.py:48-52 - is applied while the patch rows are loaded (same fp32
// operation order as k_square_pad_normalize: bit-identical to that kernel followed by the fp32 form; no fp32 NCHW batch in HBM).
// RAGGED: a packed batch of images of different sizes whose longer side is 224; image b is desc[b0 + b] = {byte offset into
// img, h, w} and its padding follows from its own h, w (one descriptor load per workgroup, the loads are the uniform ones).
struct PatchU8Args {
    const unsigned char* img;   // [B][h][w][3]
    int h, w, hp, vp, fill;     // hp / vp = left / top padding of the 224 x 224 square
    float mean[3], stdv[3];
};
struct PatchU8RaggedArgs : PatchU8Args {   // a derived struct: the uniform instantiations keep their argument layout and code
    const int64_t* desc;        // [B][3] per-image descriptors on the device
    int b0;                     // batch index of this launch's first image
};
// k_patch_embed96's staging: the 2 patch rows of block (blockIdx.x, image b) -> xin[patch][ci*16 + dy*4 + dx], as in k_patch_embed
// (which keeps its own copy of these lines, so that its code does not move)
template <bool U8, bool RAGGED>
__device__ __forceinline__ void pe_stage(const float* __restrict__ x, const std::conditional_t<RAGGED, PatchU8RaggedArgs, PatchU8Args>& u,
                                         float (*xin)[48], int b, int p0, int H, int W, int gw, int L) {
    const int py0 = p0 / gw;
    // 2 patch rows x 3 channels x 4 dy image rows of gw float4s each
    for (int i = threadIdx.x; i < 2 * 12 * gw; i += 256) {
        const int r = i / gw, px = i - r * gw;             // r = pyl*12 + ci*4 + dy
        const int pyl = r / 12, cd = r - pyl * 12, ci = cd >> 2, dy = cd & 3;
        const int py = py0 + pyl;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (py * gw + px < L) {
            if constexpr (U8) {
                PatchU8Args g = u;      // RAGGED: this image's first byte, size and padding in place of the batch's
                if constexpr (RAGGED) {
                    const int64_t* d = u.desc + (size_t)(u.b0 + b) * 3;
                    g.img = u.img + d[0]; g.h = (int)d[1]; g.w = (int)d[2];
                    g.hp = (224 - g.w) / 2; g.vp = (224 - g.h) / 2;
                }
                const unsigned char* ib = RAGGED ? g.img : g.img + (size_t)b * g.h * g.w * 3;
                const int iy = 4 * py + dy - g.vp;
                float e[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ix = 4 * px + q - g.hp;
                    int pv = g.fill;
                    if (iy >= 0 && iy < g.h && ix >= 0 && ix < g.w) pv = ib[((size_t)iy * g.w + ix) * 3 + ci];
                    e[q] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)pv, 255.0f), g.mean[ci]), g.stdv[ci]);
                }
                v = (f32x4){e[0], e[1], e[2], e[3]};
            } else {
                v = *reinterpret_cast<const f32x4*>(x + (((size_t)b * 3 + ci) * H + 4 * py + dy) * W + 4 * px);
            }
        }
        *reinterpret_cast<f32x4*>(&xin[pyl * gw + px][ci * 16 + dy * 4]) = v;
    }
}

template <bool U8, bool RAGGED = false>
__global__ __launch_bounds__(256) void k_patch_embed(const float* __restrict__ x,
                                                     const std::conditional_t<RAGGED, PatchU8RaggedArgs, PatchU8Args> u,
                                                     const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, bf16_t* __restrict__ out, int H,
                                                     int W, int gw, int L, float eps) {
    __shared__ __attribute__((aligned(16))) float xin[PE_P][48];
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * PE_P;          // PE_P == 2 * gw: the block starts at a patch-row boundary
    const int py0 = p0 / gw;
    // 2 patch rows x 3 channels x 4 dy image rows of gw float4s each
    for (int i = threadIdx.x; i < 2 * 12 * gw; i += 256) {
        const int r = i / gw, px = i - r * gw;             // r = pyl*12 + ci*4 + dy
        const int pyl = r / 12, cd = r - pyl * 12, ci = cd >> 2, dy = cd & 3;
        const int py = py0 + pyl;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (py * gw + px < L) {
            if constexpr (U8) {
                PatchU8Args g = u;      // RAGGED: this image's first byte, size and padding in place of the batch's
                if constexpr (RAGGED) {
                    const int64_t* d = u.desc + (size_t)(u.b0 + b) * 3;
                    g.img = u.img + d[0]; g.h = (int)d[1]; g.w = (int)d[2];
                    g.hp = (224 - g.w) / 2; g.vp = (224 - g.h) / 2;
                }
                const unsigned char* ib = RAGGED ? g.img : g.img + (size_t)b * g.h * g.w * 3;
                const int iy = 4 * py + dy - g.vp;
                float e[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ix = 4 * px + q - g.hp;
                    int pv = g.fill;
                    if (iy >= 0 && iy < g.h && ix >= 0 && ix < g.w) pv = ib[((size_t)iy * g.w + ix) * 3 + ci];
                    e[q] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)pv, 255.0f), g.mean[ci]), g.stdv[ci]);
                }
                v = (f32x4){e[0], e[1], e[2], e[3]};
            } else {
                v = *reinterpret_cast<const f32x4*>(x + (((size_t)b * 3 + ci) * H + 4 * py + dy) * W + 4 * px);
            }
        }
        *reinterpret_cast<f32x4*>(&xin[pyl * gw + px][ci * 16 + dy * 4]) = v;
    }
    __syncthreads();
    const int pg = threadIdx.x >> 4, cg = threadIdx.x & 15;
    float acc[PE_PPT][8];
    {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + cg * 8);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(bias + cg * 8 + 4);
#pragma unroll
        for (int p = 0; p < PE_PPT; ++p) {
            acc[p][0] = b0.x; acc[p][1] = b0.y; acc[p][2] = b0.z; acc[p][3] = b0.w;
            acc[p][4] = b1.x; acc[p][5] = b1.y; acc[p][6] = b1.z; acc[p][7] = b1.w;
        }
    }
#pragma unroll 2
    for (int k4 = 0; k4 < 48; k4 += 4) {
        f32x4 xv[PE_PPT];
#pragma unroll
        for (int p = 0; p < PE_PPT; ++p) xv[p] = *reinterpret_cast<const f32x4*>(&xin[pg * PE_PPT + p][k4]);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + (k4 + kk) * 128 + cg * 8);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(w + (k4 + kk) * 128 + cg * 8 + 4);
#pragma unroll
            for (int p = 0; p < PE_PPT; ++p) {
                const float v = xv[p][kk];
                acc[p][0] += v * w0.x; acc[p][1] += v * w0.y; acc[p][2] += v * w0.z; acc[p][3] += v * w0.w;
                acc[p][4] += v * w1.x; acc[p][5] += v * w1.y; acc[p][6] += v * w1.z; acc[p][7] += v * w1.w;
            }
        }
    }
    float g[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { g[j] = gamma[cg * 8 + j]; be[j] = beta[cg * 8 + j]; }
#pragma unroll
    for (int p = 0; p < PE_PPT; ++p) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += acc[p][j];
        const float mean = group_sum<16>(s) * (1.0f / 128.0f);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { acc[p][j] -= mean; q += acc[p][j] * acc[p][j]; }
        const float rstd = rsqrtf(group_sum<16>(q) * (1.0f / 128.0f) + eps);
        const int pp = p0 + pg * PE_PPT + p;
        if (pp < L) {
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = acc[p][j] * rstd * g[j] + be[j];
            *reinterpret_cast<u32x4*>(out + ((size_t)b * L + pp) * 128 + cg * 8) = sw_pack8(y);
        }
    }
}

// The same for embed width 96 (swin_s3_base_224): thread = (channel group of 6, patch group), LayerNorm(96) over the 16
// channel groups.  (A kernel of its own: the 128-wide one keeps its code.)
template <bool U8, bool RAGGED = false>
__global__ __launch_bounds__(256) void k_patch_embed96(const float* __restrict__ x,
                                                       const std::conditional_t<RAGGED, PatchU8RaggedArgs, PatchU8Args> u,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ bias, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, bf16_t* __restrict__ out, int H,
                                                       int W, int gw, int L, float eps) {
    constexpr int CO = 96, CPT = CO / 16;
    __shared__ __attribute__((aligned(16))) float xin[PE_P][48];
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * PE_P;
    pe_stage<U8, RAGGED>(x, u, xin, b, p0, H, W, gw, L);
    __syncthreads();
    const int pg = threadIdx.x >> 4, cg = threadIdx.x & 15;
    float acc[PE_PPT][CPT];
#pragma unroll
    for (int p = 0; p < PE_PPT; ++p)
#pragma unroll
        for (int j = 0; j < CPT; ++j) acc[p][j] = bias[cg * CPT + j];
#pragma unroll 2
    for (int k4 = 0; k4 < 48; k4 += 4) {
        f32x4 xv[PE_PPT];
#pragma unroll
        for (int p = 0; p < PE_PPT; ++p) xv[p] = *reinterpret_cast<const f32x4*>(&xin[pg * PE_PPT + p][k4]);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float wv[CPT];
#pragma unroll
            for (int j = 0; j < CPT; j += 2) {
                const float2 t = *reinterpret_cast<const float2*>(w + (k4 + kk) * CO + cg * CPT + j);
                wv[j] = t.x; wv[j + 1] = t.y;
            }
#pragma unroll
            for (int p = 0; p < PE_PPT; ++p) {
                const float v = xv[p][kk];
#pragma unroll
                for (int j = 0; j < CPT; ++j) acc[p][j] += v * wv[j];
            }
        }
    }
    float g[CPT], be[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) { g[j] = gamma[cg * CPT + j]; be[j] = beta[cg * CPT + j]; }
#pragma unroll
    for (int p = 0; p < PE_PPT; ++p) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; ++j) s += acc[p][j];
        const float mean = group_sum<16>(s) * (1.0f / CO);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; ++j) { acc[p][j] -= mean; q += acc[p][j] * acc[p][j]; }
        const float rstd = rsqrtf(group_sum<16>(q) * (1.0f / CO) + eps);
        const int pp = p0 + pg * PE_PPT + p;
        if (pp < L) {
            unsigned* o = reinterpret_cast<unsigned*>(out + ((size_t)b * L + pp) * CO + cg * CPT);
#pragma unroll
            for (int j = 0; j < CPT; j += 2)
                o[j / 2] = pack2bf(acc[p][j] * rstd * g[j] + be[j], acc[p][j + 1] * rstd * g[j + 1] + be[j + 1]);
        }
    }
}

// =====================================================================================
// LayerNorm over the channel dim of [rows][C] bf16.  LPR lanes per row, VPL 16-byte vectors per lane:
// C = LPR * VPL * 8.  MERGE: the input row is the 2x2 patch-merge concat [x(2y,2x), x(2y+1,2x), x(2y,2x+1),
// x(2y+1,2x+1)] of a [B][2*gh][2*gw][C/4] tensor (timm PatchMerging order), gathered on load.
// =====================================================================================
// STATS: write only (mean, rstd) of every row (float2 stats[rows], through `out`): the consumer GEMM applies the
// normalisation in its epilogue (Op::fuse_next), so the normalised tensor is never written or re-read.
template <int LPR, int VPL, bool MERGE, bool STATS = false>
__global__ __launch_bounds__(256) void k_layernorm(const bf16_t* __restrict__ in, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, bf16_t* __restrict__ out, long rows,
                                                   int gh, int gw, float eps) {
    constexpr int C = LPR * VPL * 8;
    constexpr int RPB = 256 / LPR;   // rows per block
    const int sub = threadIdx.x % LPR;
    const long row = (long)blockIdx.x * RPB + threadIdx.x / LPR;
    const bool live = row < rows;
    float v[VPL][8];
    const bf16_t* src[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int vec = sub + i * LPR;   // vector index within the row
        if (MERGE) {
            constexpr int C4 = C / 4;                 // source channels
            const int part = (vec * 8) / C4, off = (vec * 8) - part * C4;
            const long r = live ? row : 0;
            const long bimg = r / ((long)gh * gw);
            const int rem = (int)(r - bimg * gh * gw);
            const int oy = rem / gw, ox = rem - oy * gw;
            const int sy = 2 * oy + (part & 1), sx = 2 * ox + (part >> 1);
            src[i] = in + ((bimg * (2 * gh) + sy) * (2 * gw) + sx) * (long)C4 + off;
        } else {
            src[i] = in + (live ? row : 0) * (long)C + vec * 8;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        sw_unpack8(*reinterpret_cast<const u32x4*>(src[i]), v[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[i][j];
    }
    const float mean = group_sum<LPR>(s) * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[i][j] -= mean; q += v[i][j] * v[i][j]; }
    const float rstd = rsqrtf(group_sum<LPR>(q) * (1.0f / C) + eps);
    if (!live) return;
    if (STATS) {
        if (sub == 0) { float* st = reinterpret_cast<float*>(out) + row * 2; st[0] = mean; st[1] = rstd; }
        return;
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c0 = (sub + i * LPR) * 8;
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c0), g1 = *reinterpret_cast<const f32x4*>(gamma + c0 + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c0), b1 = *reinterpret_cast<const f32x4*>(beta + c0 + 4);
        float y[8] = {v[i][0] * rstd * g0.x + b0.x, v[i][1] * rstd * g0.y + b0.y, v[i][2] * rstd * g0.z + b0.z,
                      v[i][3] * rstd * g0.w + b0.w, v[i][4] * rstd * g1.x + b1.x, v[i][5] * rstd * g1.y + b1.y,
                      v[i][6] * rstd * g1.z + b1.z, v[i][7] * rstd * g1.w + b1.w};
        *reinterpret_cast<u32x4*>(out + row * (long)C + c0) = sw_pack8(y);
    }
}

template <bool MERGE, bool STATS = false>
static int launch_ln(const bf16_t* in, const float* g, const float* b, bf16_t* out, long rows, int C, int gh, int gw,
                     float eps, hipStream_t st) {
#define LN_CASE(LPR, VPL)                                                                                  \
    hipLaunchKernelGGL((k_layernorm<LPR, VPL, MERGE, STATS>), dim3((unsigned)cdiv(rows, 256 / LPR)), dim3(256), 0, st, in, g, b, \
                       out, rows, gh, gw, eps)
    switch (C) {
        case 96: LN_CASE(4, 3); break;      // (96 .. 1536 with three vectors per lane: swin_s3_base_224's widths)
        case 192: LN_CASE(8, 3); break;
        case 384: LN_CASE(16, 3); break;
        case 768: LN_CASE(32, 3); break;
        case 1536: LN_CASE(64, 3); break;
        case 128: LN_CASE(16, 1); break;
        case 256: LN_CASE(32, 1); break;
        case 512: LN_CASE(64, 1); break;
        case 1024: LN_CASE(64, 2); break;
        case 2048: LN_CASE(64, 4); break;
        default: set_error("layernorm: unsupported width %d", C); return ERR_UNSUPPORTED;
    }
#undef LN_CASE
    MI355_LAUNCH_CHECK();
    return OK;
}

// final LayerNorm(C = 1024) + mean over the L tokens of an image -> pooled fp32 (+ bf16 copy).  One block per image;
// wave w normalises tokens w, w+4, ... and the four per-wave partial sums are added in wave order.
__global__ __launch_bounds__(256) void k_ln_token_mean(const bf16_t* __restrict__ in, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ pooled,
                                                       bf16_t* __restrict__ pooled_bf16, int L, float eps) {
    constexpr int C = 1024;
    __shared__ float part[4][C];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int t = wave; t < L; t += 4) {
        const bf16_t* src = in + ((size_t)b * L + t) * C;
        float v[2][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            sw_unpack8(*reinterpret_cast<const u32x4*>(src + (lane + i * 64) * 8), v[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[i][j];
        }
        const float mean = group_sum<64>(s) * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[i][j] -= mean; q += v[i][j] * v[i][j]; }
        const float rstd = rsqrtf(group_sum<64>(q) * (1.0f / C) + eps);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = (lane + i * 64) * 8 + j;
                acc[i][j] += v[i][j] * rstd * gamma[c] + beta[c];
            }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) part[wave][(lane + i * 64) * 8 + j] = acc[i][j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const float m = (part[0][c] + part[1][c] + part[2][c] + part[3][c]) / (float)L;
        pooled[(size_t)b * C + c] = m;
        pooled_bf16[(size_t)b * C + c] = f2bf(m);
    }
}

// The same for C = 768 (swin_s3_base_224): a lane holds vectors lane and lane + 64 (the second only for lane < 32).
// (A kernel of its own: the 1024-wide one keeps its code.)
__global__ __launch_bounds__(256) void k_ln_token_mean768(const bf16_t* __restrict__ in, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ pooled,
                                                          bf16_t* __restrict__ pooled_bf16, int L, float eps) {
    constexpr int C = 768, NV = C / 8;
    __shared__ float part[4][C];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int t = wave; t < L; t += 4) {
        const bf16_t* src = in + ((size_t)b * L + t) * C;
        float v[2][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int vec = lane + i * 64;
            if (vec < NV) sw_unpack8(*reinterpret_cast<const u32x4*>(src + vec * 8), v[i]);
            else
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[i][j];
        }
        const float mean = group_sum<64>(s) * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (lane + i * 64 < NV)
#pragma unroll
                for (int j = 0; j < 8; ++j) { v[i][j] -= mean; q += v[i][j] * v[i][j]; }
        const float rstd = rsqrtf(group_sum<64>(q) * (1.0f / C) + eps);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (lane + i * 64 < NV)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = (lane + i * 64) * 8 + j;
                    acc[i][j] += v[i][j] * rstd * gamma[c] + beta[c];
                }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (lane + i * 64 < NV)
#pragma unroll
            for (int j = 0; j < 8; ++j) part[wave][(lane + i * 64) * 8 + j] = acc[i][j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const float m = (part[0][c] + part[1][c] + part[2][c] + part[3][c]) / (float)L;
        pooled[(size_t)b * C + c] = m;
        pooled_bf16[(size_t)b * C + c] = f2bf(m);
    }
}

// =====================================================================================
// window attention.  qkv [B][L][3C] bf16 (channel = which*C + head*32 + d), out [B][L][C] bf16.
// bias [heads][49][64] fp32 (dense relative-position bias, key dim padded to 64).
// =====================================================================================
constexpr int WA_N = 49;       // tokens per 7x7 window
constexpr int WA_VLD = 72;     // Vt row stride (keys) in bf16

__global__ __launch_bounds__(256) void k_win_attn(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                  bf16_t* __restrict__ out, int res, int C, int heads, int shift,
                                                  long ntasks, float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t Vt_all[4][32 * WA_VLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long task = (long)blockIdx.x * 4 + wave;
    if (task >= ntasks) return;          // whole wave exits together; no block-level barrier below
    bf16_t* Vt = Vt_all[wave];
    const int nwx = res / 7, nW = nwx * nwx;
    const int h = (int)(task % heads);
    const long bw = task / heads;
    const int win = (int)(bw % nW);
    const long b = bw / nW;
    const int wy = win / nwx, wx = win - wy * nwx;
    const int L = res * res, C3 = 3 * C;
    const bf16_t* base = qkv + (size_t)b * L * C3 + h * 32;

    // in-window index -> image token (undoing the cyclic shift) and shifted-frame region label
    auto token_of = [&](int i) {
        const int iy = i / 7, ix = i - iy * 7;
        int y = wy * 7 + iy + shift, x = wx * 7 + ix + shift;
        if (y >= res) y -= res;
        if (x >= res) x -= res;
        return y * res + x;
    };
    auto label_of = [&](int i) {
        const int iy = i / 7, ix = i - iy * 7;
        const int y = wy * 7 + iy, x = wx * 7 + ix;
        const int rh = y < res - 7 ? 0 : (y < res - shift ? 1 : 2);
        const int rw = x < res - 7 ? 0 : (x < res - shift ? 1 : 2);
        return rh * 3 + rw;
    };

    const int fr = lane & 15, fq = lane >> 4;

    // ---- V^T -> LDS: Vt[d][key]; keys >= 49 are zero
    for (int i = lane; i < 32 * WA_VLD / 2; i += 64) reinterpret_cast<unsigned*>(Vt)[i] = 0u;
    for (int c = lane; c < WA_N * 4; c += 64) {
        const int key = c >> 2, dp = (c & 3) * 8;
        const u32x4 v = *reinterpret_cast<const u32x4*>(base + (size_t)token_of(key) * C3 + 2 * C + dp);
        const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(dp + j) * WA_VLD + key] = e[j];
    }

    // ---- per query tile u: S^T = K Q^T (keys on the MFMA rows), bias + mask + softmax, O^T = V^T P^T, store.
    // Working one 16-query tile at a time keeps ~90 VGPRs live (the all-at-once form needed 176 -> 2 waves/SIMD).
    bf16x8 kf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = t * 16 + fr;
        u32x4 kv = {0u, 0u, 0u, 0u};
        if (i < WA_N) kv = *reinterpret_cast<const u32x4*>(base + (size_t)token_of(i) * C3 + C + fq * 8);
        kf[t] = *reinterpret_cast<bf16x8*>(&kv);
    }
    const float* bh = bias + (size_t)h * WA_N * 64;
#pragma unroll 1
    for (int u = 0; u < 4; ++u) {
        const int qi = u * 16 + fr;
        const int qc = qi < WA_N ? qi : WA_N - 1;     // clamp padded queries to a valid row (result discarded)
        const int qtok = token_of(qc);
        const u32x4 qv = *reinterpret_cast<const u32x4*>(base + (size_t)qtok * C3 + fq * 8);
        const bf16x8 qf = *reinterpret_cast<const bf16x8*>(&qv);
        f32x4 s[4];   // [key tile t]; lane: query = 16u + fr, keys = 16t + 4*fq + r
#pragma unroll
        for (int t = 0; t < 4; ++t)
            s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t], qf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);

        const int ql = shift > 0 ? label_of(qc) : 0;
        float v[4][4];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k0 = t * 16 + fq * 4;
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bh + (size_t)qc * 64 + k0);
            const float sv[4] = {s[t].x, s[t].y, s[t].z, s[t].w};
            const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + r;
                float x = sv[r] * scale + bv[r];
                if (shift > 0 && key < WA_N && label_of(key) != ql) x += -100.0f;
                if (key >= WA_N) x = -INFINITY;
                v[t][r] = x;
                mx = fmaxf(mx, x);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[t][r] = __builtin_amdgcn_exp2f((v[t][r] - mx) * 1.4426950408889634f);
                sum += v[t][r];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = __builtin_amdgcn_rcpf(sum);
        bf16x8 pf[2];   // P^T in B-operand layout for the two 32-key k-steps
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 pk;
            pk.x = pack2bf(v[2 * ks][0] * inv, v[2 * ks][1] * inv);
            pk.y = pack2bf(v[2 * ks][2] * inv, v[2 * ks][3] * inv);
            pk.z = pack2bf(v[2 * ks + 1][0] * inv, v[2 * ks + 1][1] * inv);
            pk.w = pack2bf(v[2 * ks + 1][2] * inv, v[2 * ks + 1][3] * inv);
            pf[ks] = *reinterpret_cast<bf16x8*>(&pk);
        }

        // O^T = V^T P^T : A rows = d (two 16-row tiles), k = keys in the SAME permuted order as pf:
        // element j of lane group fq in k-step ks is key 16*(2ks + (j>>2)) + 4*fq + (j&3)
        f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int vt = 0; vt < 2; ++vt) {
                const bf16_t* vr = Vt + (vt * 16 + fr) * WA_VLD + 32 * ks + 4 * fq;
                u32x4 a;
                const u32x2 lo = *reinterpret_cast<const u32x2*>(vr);
                const u32x2 hi = *reinterpret_cast<const u32x2*>(vr + 16);
                a.x = lo.x; a.y = lo.y; a.z = hi.x; a.w = hi.y;
                o[vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8*>(&a), pf[ks], o[vt], 0, 0, 0);
            }
        }
        // store: lane holds query 16u + fr, d = 16vt + 4*fq + r
        if (qi < WA_N) {
            bf16_t* orow = out + ((size_t)b * L + qtok) * C + h * 32 + fq * 4;
#pragma unroll
            for (int vt = 0; vt < 2; ++vt) {
                u32x2 w;
                w.x = pack2bf(o[vt].x, o[vt].y);
                w.y = pack2bf(o[vt].z, o[vt].w);
                *reinterpret_cast<u32x2*>(orow + vt * 16) = w;
            }
        }
    }
}

// =====================================================================================
// 14x14 window attention (swin_s3_base_224's 14x14 stage: one window per image, no shift, no mask).
// qkv / out as above; table [heads][27*27] fp32 (the head-major copy of timm's relative_position_bias_table).
// One workgroup of 4 waves per (image, window, head): 196 tokens padded to 208 = 13 tiles of 16.  K ([key][d]), V^T
// ([d][key]) and the head's 729-entry bias table are staged in LDS once (31 KB), behind
// one barrier that every wave reaches.  Wave w then takes query strips w, w+4, ...: S^T = K Q^T for all 13 key tiles
// (as in k_win_attn: keys on the MFMA rows, a lane holds 52 keys of one query), the bias is read from the table at
// (qy-ky+13)*27 + (qx-kx+13), padded keys are -inf, and the whole row is in registers, so the softmax is the exact
// two-pass form.  P (rounded to bf16) x V runs in 7 k-steps of 32 keys; the 14th key tile is zero on both sides.
// =====================================================================================
constexpr int WB_WS = 14, WB_N = 196, WB_T = 13;   // window side, tokens per window, 16-key tiles
constexpr int WB_KS = 7;                            // 32-key k-steps of P V
constexpr int WB_VLD = WB_KS * 32 + 8;              // Vt row stride (keys) in bf16
constexpr int WB_TAB = 27 * 27;                     // (2*14-1)^2 relative positions

__global__ __launch_bounds__(256) void k_win_attn14(const bf16_t* __restrict__ qkv, const float* __restrict__ table,
                                                    bf16_t* __restrict__ out, int res, int C, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[WB_T * 16 * 32];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[32 * WB_VLD];
    __shared__ float tab[WB_TAB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long task = blockIdx.x;
    const int nwx = res / WB_WS, nW = nwx * nwx;
    const int h = (int)(task % heads);
    const long bw = task / heads;
    const int win = (int)(bw % nW);
    const long b = bw / nW;
    const int wy = win / nwx, wx = win - wy * nwx;
    const int L = res * res, C3 = 3 * C;
    const bf16_t* base = qkv + (size_t)b * L * C3 + h * 32;
    auto token_of = [&](int i) {
        const int iy = i / WB_WS, ix = i - iy * WB_WS;
        return (wy * WB_WS + iy) * res + wx * WB_WS + ix;
    };

    // ---- stage: K rows and V^T columns (keys >= 196 zero) and the head's table
    for (int c = threadIdx.x; c < WB_T * 16 * 4; c += 256) {
        const int key = c >> 2, dp = (c & 3) * 8;
        u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
        if (key < WB_N) {
            const bf16_t* r = base + (size_t)token_of(key) * C3 + dp;
            kv = *reinterpret_cast<const u32x4*>(r + C);
            vv = *reinterpret_cast<const u32x4*>(r + 2 * C);
        }
        *reinterpret_cast<u32x4*>(&Ks[key * 32 + dp]) = kv;
        const bf16_t* e = reinterpret_cast<const bf16_t*>(&vv);
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(dp + j) * WB_VLD + key] = e[j];
    }
    for (int i = threadIdx.x; i < 32 * 16; i += 256) Vt[(i >> 4) * WB_VLD + WB_T * 16 + (i & 15)] = f2bf(0.f);   // keys 208..223
    for (int i = threadIdx.x; i < WB_TAB; i += 256) tab[i] = table[(size_t)h * WB_TAB + i];
    __syncthreads();

    const int fr = lane & 15, fq = lane >> 4;
#pragma unroll 1
    for (int u = wave; u < WB_T; u += 4) {
        const int qi = u * 16 + fr;
        const int qc = qi < WB_N ? qi : WB_N - 1;     // clamp padded queries to a valid row (result discarded)
        const int qtok = token_of(qc);
        const u32x4 qv = *reinterpret_cast<const u32x4*>(base + (size_t)qtok * C3 + fq * 8);
        const bf16x8 qf = *reinterpret_cast<const bf16x8*>(&qv);
        const int qy = qc / WB_WS, qb = (qy + 13) * 27 + (qc - qy * WB_WS) + 13;
        // kz == 0, but not provably so: it keeps the K fragment reads and the bias offsets (104 values that do not depend on the
        // strip) inside this loop; hoisted out of it they stay live across it and spill (measured: 161 spilled VGPRs)
        const int kz = __builtin_amdgcn_readfirstlane(u) - u;
        float v[WB_T][4];   // [key tile t][r]: query 16u + fr, key 16t + 4fq + r
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < WB_T; ++t) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(t * 16 + fr + kz) * 32 + fq * 8]);
            const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            const int k0 = t * 16 + fq * 4 + kz;
            const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // key k0 + r at (ky, kx) = (k / 14, k % 14): table row (qy-ky+13)*27 + (qx-kx+13) = qb - (k + 13 ky);
                // padded keys are -inf and read key 195's row (inside the table).  (k * 4682) >> 16 == k / 14 for k < 196.
                const int k = t == WB_T - 1 ? min(k0 + r, WB_N - 1) : k0 + r, ky = (k * 4682) >> 16;
                float x = sv[r] * scale + tab[qb - k - 13 * ky];
                if (t == WB_T - 1 && k0 + r >= WB_N) x = -INFINITY;
                v[t][r] = x;
                mx = fmaxf(mx, x);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < WB_T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[t][r] = __builtin_amdgcn_exp2f((v[t][r] - mx) * 1.4426950408889634f);
                sum += v[t][r];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = __builtin_amdgcn_rcpf(sum);

        // O^T = V^T P^T, k permuted as in k_win_attn: element j of lane group fq in k-step ks is key 16*(2ks + (j>>2)) + 4fq + (j&3)
        f32x4 o[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < WB_KS; ++ks) {
            u32x4 pk;
            pk.x = pack2bf(v[2 * ks][0] * inv, v[2 * ks][1] * inv);
            pk.y = pack2bf(v[2 * ks][2] * inv, v[2 * ks][3] * inv);
            if (2 * ks + 1 < WB_T) {
                pk.z = pack2bf(v[2 * ks + 1][0] * inv, v[2 * ks + 1][1] * inv);
                pk.w = pack2bf(v[2 * ks + 1][2] * inv, v[2 * ks + 1][3] * inv);
            } else {
                pk.z = 0u; pk.w = 0u;
            }
            const bf16x8 pf = *reinterpret_cast<bf16x8*>(&pk);
#pragma unroll
            for (int vt = 0; vt < 2; ++vt) {
                const bf16_t* vr = Vt + (vt * 16 + fr) * WB_VLD + 32 * ks + 4 * fq;
                u32x4 a;
                const u32x2 lo = *reinterpret_cast<const u32x2*>(vr);
                const u32x2 hi = *reinterpret_cast<const u32x2*>(vr + 16);
                a.x = lo.x; a.y = lo.y; a.z = hi.x; a.w = hi.y;
                o[vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<bf16x8*>(&a), pf, o[vt], 0, 0, 0);
            }
        }
        if (qi < WB_N) {
            bf16_t* orow = out + ((size_t)b * L + qtok) * C + h * 32 + fq * 4;
#pragma unroll
            for (int vt = 0; vt < 2; ++vt) {
                u32x2 w;
                w.x = pack2bf(o[vt].x, o[vt].y);
                w.y = pack2bf(o[vt].z, o[vt].w);
                *reinterpret_cast<u32x2*>(orow + vt * 16) = w;
            }
        }
    }
}

// =====================================================================================
// packing + execution hooks used by model.hip
// =====================================================================================
static inline uint16_t f2bf_h(float f) { return f2bf_host(f); }

// relative_position_bias_table [(2*7-1)^2][heads] -> the dense [heads][49][64] bias k_win_attn reads (key dim padded to 64 with
// zeros).  Shared by the model pack and mi355_window_attention, so the op-level test covers the packing too.
static void swin_dense_rel_bias(const float* table, int heads, float* dense) {
    constexpr int ws = 7;
    for (int hh = 0; hh < heads; ++hh)
        for (int i = 0; i < WA_N; ++i)
            for (int j = 0; j < 64; ++j) {
                float v = 0.f;
                if (j < WA_N) {
                    // relative_position_index[i][j] (timm WindowAttention.__init__)
                    const int dy = i / ws - j / ws + ws - 1, dx = i % ws - j % ws + ws - 1;
                    v = table[(size_t)(dy * (2 * ws - 1) + dx) * heads + hh];
                }
                dense[((size_t)hh * WA_N + i) * 64 + j] = v;
            }
}

// relative_position_bias_table [(2*14-1)^2][heads] -> the head-major [heads][729] copy k_win_attn14 stages per head.  Shared by the
// model pack and mi355_window_attention_ws.
static void swin_headmajor_rel_bias(const float* table, int heads, float* out) {
    for (int hh = 0; hh < heads; ++hh)
        for (int i = 0; i < WB_TAB; ++i) out[(size_t)hh * WB_TAB + i] = table[(size_t)i * heads + hh];
}

static int launch_win_attn14(const bf16_t* qkv, const float* table, bf16_t* out, long B, int res, int C, int heads, hipStream_t st) {
    const long ntasks = B * (res / WB_WS) * (res / WB_WS) * heads;
    MI355_REQUIRE(ntasks >= 1 && ntasks < (1l << 31), "win_attn14: grid of %ld tasks too large", ntasks);
    hipLaunchKernelGGL(k_win_attn14, dim3((unsigned)ntasks), dim3(256), 0, st, qkv, table, out, res, C, heads,
                       0.17677669529663687f /* 32^-0.5 */);
    MI355_LAUNCH_CHECK();
    return OK;
}

static int launch_win_attn(const bf16_t* qkv, const float* bias_dense, bf16_t* out, long B, int res, int C, int heads, int shift,
                           hipStream_t st) {
    const long ntasks = B * (res / 7) * (res / 7) * heads;
    MI355_REQUIRE(ntasks >= 1 && ntasks / 4 < (1l << 31), "win_attn: grid of %ld tasks too large", ntasks);
    hipLaunchKernelGGL(k_win_attn, dim3((unsigned)cdiv(ntasks, 4)), dim3(256), 0, st, qkv, bias_dense, out, res, C, heads, shift, ntasks,
                       0.17677669529663687f /* 32^-0.5 */);
    MI355_LAUNCH_CHECK();
    return OK;
}

// patch_embed.proj.weight [co_n][3][4][4] -> the [48][co_n] fp32 matrix k_patch_embed* read (k = ci*16 + dy*4 + dx), values rounded
// to bf16.  Shared by the model pack and mi355_swin_patch_embed.
static void swin_patch_weight(const float* w, int co_n, float* W) {
    for (int co = 0; co < co_n; ++co)
        for (int k = 0; k < 48; ++k) W[(size_t)k * co_n + co] = bf_round_host(w[(size_t)co * 48 + k]);
}

// The uint8 operand block of k_patch_embed*: the SquarePad offsets of an h x w image in the 224 x 224 square (ragged batches take
// them per image from desc, in the kernel).  Shared by swin_exec and mi355_swin_patch_embed.
static PatchU8RaggedArgs patch_u8_args(const unsigned char* img, int h, int w, int fill, const float* mean, const float* stdv,
                                       const int64_t* desc, int b0) {
    PatchU8RaggedArgs r{};
    r.img = img; r.h = h; r.w = w; r.hp = (224 - w) / 2; r.vp = (224 - h) / 2; r.fill = fill;
    for (int c = 0; c < 3; ++c) { r.mean[c] = mean[c]; r.stdv[c] = stdv[c]; }
    r.desc = desc; r.b0 = b0;
    return r;
}

// x: fp32 [nb][3][H][W], or NULL with r.img the uint8 batch (ragged when r.desc is set); out [nb][(H/4)*(W/4)][embed] bf16
static int launch_patch_embed(const float* x, const PatchU8RaggedArgs& r, int embed, const float* w, const float* bias, const float* g,
                              const float* be, bf16_t* out, int nb, int H, int W, float eps, hipStream_t st) {
    const int gw = W / 4, L = gw * (H / 4);
    MI355_REQUIRE(2 * gw == PE_P, "patch_embed: kernel is laid out for 56 patches per row");
    MI355_REQUIRE(embed == 128 || embed == 96, "patch_embed: width %d unsupported", embed);
    const PatchU8Args& u = r;
    const dim3 grid(cdiv(L, PE_P), nb);
    const bool w96 = embed == 96;
    if (!x) {            // uint8 images: SquarePad + ToTensor + Normalize fused into the patch loads (mi355_model_forward_u8)
        if (r.desc && w96)
            hipLaunchKernelGGL((k_patch_embed96<true, true>), grid, dim3(256), 0, st, (const float*)nullptr, r, w, bias, g, be, out, H, W,
                               gw, L, eps);
        else if (r.desc)
            hipLaunchKernelGGL((k_patch_embed<true, true>), grid, dim3(256), 0, st, (const float*)nullptr, r, w, bias, g, be, out, H, W,
                               gw, L, eps);
        else if (w96)
            hipLaunchKernelGGL(k_patch_embed96<true>, grid, dim3(256), 0, st, (const float*)nullptr, u, w, bias, g, be, out, H, W, gw, L,
                               eps);
        else
            hipLaunchKernelGGL(k_patch_embed<true>, grid, dim3(256), 0, st, (const float*)nullptr, u, w, bias, g, be, out, H, W, gw, L, eps);
    } else if (w96) {
        hipLaunchKernelGGL(k_patch_embed96<false>, grid, dim3(256), 0, st, x, u, w, bias, g, be, out, H, W, gw, L, eps);
    } else {
        hipLaunchKernelGGL(k_patch_embed<false>, grid, dim3(256), 0, st, x, u, w, bias, g, be, out, H, W, gw, L, eps);
    }
    MI355_LAUNCH_CHECK();
    return OK;
}

static int launch_ln_token_mean(const bf16_t* in, const float* g, const float* be, float* pooled, bf16_t* pooled_bf16, int nb, int L,
                                int C, float eps, hipStream_t st) {
    MI355_REQUIRE(C == 1024 || C == 768, "token_mean: width %d unsupported", C);
    if (C == 768)
        hipLaunchKernelGGL(k_ln_token_mean768, dim3(nb), dim3(256), 0, st, in, g, be, pooled, pooled_bf16, L, eps);
    else
        hipLaunchKernelGGL(k_ln_token_mean, dim3(nb), dim3(256), 0, st, in, g, be, pooled, pooled_bf16, L, eps);
    MI355_LAUNCH_CHECK();
    return OK;
}

int swin_pack(Packer& pk, Op& op) {
    auto put_vec = [&](const std::string& name, int n, size_t& off) -> int {
        const TensorSpec* t = pk.get(name);
        if (!t) return ERR_STATE;
        MI355_REQUIRE(t->numel() == n, "pack: %s has %lld elements, expected %d", name.c_str(), (long long)t->numel(), n);
        off = pk.alloc((size_t)n * 4);
        memcpy(pk.blob.data() + off, t->data.data(), (size_t)n * 4);
        return OK;
    };
    switch (op.kind) {
        case OP_PATCH_EMBED: {
            const TensorSpec* w = pk.get(op.w_name);
            if (!w) return ERR_STATE;
            const int co_n = op.cout;   // 128 (swin_base) or 96 (swin_s3_base): [48][co_n]
            MI355_REQUIRE((co_n == 128 || co_n == 96) && w->numel() == co_n * 48, "pack: %s shape", op.w_name.c_str());
            op.w_off = pk.alloc((size_t)48 * co_n * 4);
            swin_patch_weight(w->data.data(), co_n, (float*)(pk.blob.data() + op.w_off));
            if (int e = put_vec(op.bias_name, co_n, op.b_off)) return e;
            if (int e = put_vec(op.w2_name, co_n, op.w2_off)) return e;
            return put_vec(op.bias2_name, co_n, op.b2_off);
        }
        case OP_LAYERNORM: case OP_PATCH_MERGE_LN: case OP_TOKEN_MEAN: {
            if (int e = put_vec(op.w_name, op.cout, op.w_off)) return e;
            return put_vec(op.bias_name, op.cout, op.b_off);
        }
        case OP_WINATTN: {
            const TensorSpec* t = pk.get(op.aux_name);
            if (!t) return ERR_STATE;
            const int ws = op.window, nh = op.heads, N = ws * ws;
            if (ws == WB_WS) {   // 14x14 windows: the head-major table, indexed in the kernel (a dense bias would be 2 MB a block)
                MI355_REQUIRE(t->numel() == (int64_t)WB_TAB * nh, "pack: %s shape", op.aux_name.c_str());
                op.aux_off = pk.alloc((size_t)nh * WB_TAB * 4);
                swin_headmajor_rel_bias(t->data.data(), nh, (float*)(pk.blob.data() + op.aux_off));
                return OK;
            }
            MI355_REQUIRE(ws == 7 && t->numel() == (int64_t)(2 * ws - 1) * (2 * ws - 1) * nh, "pack: %s shape", op.aux_name.c_str());
            op.aux_off = pk.alloc((size_t)nh * N * 64 * 4);
            swin_dense_rel_bias(t->data.data(), nh, (float*)(pk.blob.data() + op.aux_off));
            return OK;
        }
        default:
            set_error("pack: unknown op kind %d", (int)op.kind);
            return ERR_STATE;
    }
}

int swin_exec(const Op& op, const Step& s, ExecCtx& cx) {
    switch (op.kind) {
        case OP_PATCH_EMBED: {
            MI355_REQUIRE(s.in.h == 224 && s.in.w == 224, "swin needs 224x224 input");
            const float *w = (const float*)cx.w(op.w_off), *bias = (const float*)cx.w(op.b_off), *g = (const float*)cx.w(op.w2_off),
                        *be = (const float*)cx.w(op.b2_off);
            bf16_t* out = (bf16_t*)cx.slot_ptr(op.out);
            PatchU8RaggedArgs r{};
            if (const U8Source* u = cx.u8) {   // uint8 images: SquarePad + ToTensor + Normalize fused into the patch loads (mi355_model_forward_u8)
                MI355_REQUIRE(!u->conv_w, "swin: the conv_input pre-stem belongs to the convolutional backbones");
                MI355_REQUIRE(std::max(u->h, u->w) == 224, "swin needs images whose longer side is 224 (got %dx%d)", u->h, u->w);
                r = patch_u8_args(cx.x_u8(), u->h, u->w, u->fill, u->mean, u->stdv, u->desc, cx.b0);
            }
            return launch_patch_embed(cx.u8 ? nullptr : cx.x, r, op.cout, w, bias, g, be, out, cx.nb, s.in.h, s.in.w, op.ln_eps, cx.st);
        }
        case OP_LAYERNORM: {
            const long rows = (long)cx.nb * op.tokens_h * op.tokens_h;
            // folded into the next GEMM (the plan decides, resolve_plan in model.hip): only the row statistics are left here
            if (s.how == MI355_PLAN_LN_STATS)
                return launch_ln<false, true>((const bf16_t*)cx.slot_ptr(op.in), nullptr, nullptr, (bf16_t*)cx.slot_ptr(SLOT_LNSTATS),
                                              rows, op.cout, 0, 0, op.ln_eps, cx.st);
            return launch_ln<false>((const bf16_t*)cx.slot_ptr(op.in), (const float*)cx.w(op.w_off), (const float*)cx.w(op.b_off),
                                    (bf16_t*)cx.slot_ptr(op.out), rows, op.cout, 0, 0, op.ln_eps, cx.st);
        }
        case OP_PATCH_MERGE_LN: {
            const long rows = (long)cx.nb * op.tokens_h * op.tokens_h;
            return launch_ln<true>((const bf16_t*)cx.slot_ptr(op.in), (const float*)cx.w(op.w_off), (const float*)cx.w(op.b_off),
                                   (bf16_t*)cx.slot_ptr(op.out), rows, op.cout, op.tokens_h, op.tokens_h, op.ln_eps, cx.st);
        }
        case OP_WINATTN: {
            MI355_REQUIRE(op.cout == op.heads * 32, "win_attn: head_dim must be 32");
            if (op.window == WB_WS) {
                MI355_REQUIRE(op.shift == 0 && op.tokens_h % WB_WS == 0, "win_attn14: res %d shift %d unsupported", op.tokens_h, op.shift);
                return launch_win_attn14((const bf16_t*)cx.slot_ptr(op.in), (const float*)cx.w(op.aux_off), (bf16_t*)cx.slot_ptr(op.out),
                                         cx.nb, op.tokens_h, op.cout, op.heads, cx.st);
            }
            return launch_win_attn((const bf16_t*)cx.slot_ptr(op.in), (const float*)cx.w(op.aux_off), (bf16_t*)cx.slot_ptr(op.out),
                                   cx.nb, op.tokens_h, op.cout, op.heads, op.shift, cx.st);
        }
        case OP_TOKEN_MEAN: {
            return launch_ln_token_mean((const bf16_t*)cx.slot_ptr(op.in), (const float*)cx.w(op.w_off), (const float*)cx.w(op.b_off),
                                        (float*)cx.slot_ptr(SLOT_POOLED), (bf16_t*)cx.slot_ptr(SLOT_POOLED_BF16), cx.nb,
                                        op.tokens_h * op.tokens_h, op.cin, op.ln_eps, cx.st);
        }
        default:
            set_error("exec: unknown op kind %d", (int)op.kind);
            return ERR_STATE;
    }
}

}  // namespace mi355

extern "C" int mi355_window_attention(const void* qkv, const float* bias_table, void* out, int B, int res, int C, int heads, int shift,
                                      void* stream) {
    using namespace mi355;
    MI355_REQUIRE(qkv && bias_table && out, "window_attention: null pointer");
    MI355_REQUIRE(B >= 1 && res >= 7 && res % 7 == 0 && res <= 7 * 1024, "window_attention: bad shape B=%d res=%d (res a multiple of 7)", B,
                  res);
    MI355_REQUIRE(heads >= 1 && heads <= 1024 && C == 32 * heads, "window_attention: C=%d must be 32 * heads (heads=%d)", C, heads);
    MI355_REQUIRE(shift == 0 || (shift == 3 && res > 7), "window_attention: shift %d (0, or 3 when res > 7)", shift);
    MI355_REQUIRE((size_t)B * res * res * 3 * C < ((size_t)1 << 40), "window_attention: tensor too large");
    MI355_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)bias_table % 4 == 0,
                  "window_attention: qkv and out must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const size_t ntab = (size_t)13 * 13 * heads, ndense = (size_t)heads * WA_N * 64;
    std::vector<float> tab(ntab), dense(ndense);
    MI355_CHECK_HIP(hipMemcpyAsync(tab.data(), bias_table, ntab * 4, hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    swin_dense_rel_bias(tab.data(), heads, dense.data());
    void* d = nullptr;
    MI355_CHECK_HIP(hipMalloc(&d, ndense * 4));
    int e = hipMemcpyAsync(d, dense.data(), ndense * 4, hipMemcpyHostToDevice, st) == hipSuccess ? OK : ERR_HIP;
    if (e) set_error("window_attention: bias upload failed");
    else e = launch_win_attn((const bf16_t*)qkv, (const float*)d, (bf16_t*)out, B, res, C, heads, shift, st);
    if (hipStreamSynchronize(st) != hipSuccess && !e) {
        set_error("window_attention: stream synchronisation failed");
        e = ERR_HIP;
    }
    MI355_CHECK_HIP(hipFree(d));
    return e;
}

extern "C" int mi355_window_attention_ws(const void* qkv, const float* bias_table, void* out, int B, int res, int C, int heads, int window,
                                         int shift, void* stream) {
    using namespace mi355;
    MI355_REQUIRE(window == 7 || window == WB_WS, "window_attention_ws: window %d (7 or 14)", window);
    if (window == 7) return mi355_window_attention(qkv, bias_table, out, B, res, C, heads, shift, stream);
    MI355_REQUIRE(qkv && bias_table && out, "window_attention_ws: null pointer");
    MI355_REQUIRE(B >= 1 && res >= WB_WS && res % WB_WS == 0 && res <= WB_WS * 512,
                  "window_attention_ws: bad shape B=%d res=%d (res a multiple of 14)", B, res);
    MI355_REQUIRE(heads >= 1 && heads <= 1024 && C == 32 * heads, "window_attention_ws: C=%d must be 32 * heads (heads=%d)", C, heads);
    MI355_REQUIRE(shift == 0, "window_attention_ws: shift %d (14x14 windows take shift 0 only)", shift);
    MI355_REQUIRE((size_t)B * res * res * 3 * C < ((size_t)1 << 40), "window_attention_ws: tensor too large");
    MI355_REQUIRE((size_t)B * (res / WB_WS) * (res / WB_WS) * heads < ((size_t)1 << 31), "window_attention_ws: grid too large");
    MI355_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)bias_table % 4 == 0,
                  "window_attention_ws: qkv and out must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const size_t ntab = (size_t)WB_TAB * heads;
    std::vector<float> tab(ntab), hm(ntab);
    MI355_CHECK_HIP(hipMemcpyAsync(tab.data(), bias_table, ntab * 4, hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    swin_headmajor_rel_bias(tab.data(), heads, hm.data());
    void* d = nullptr;
    MI355_CHECK_HIP(hipMalloc(&d, ntab * 4));
    int e = hipMemcpyAsync(d, hm.data(), ntab * 4, hipMemcpyHostToDevice, st) == hipSuccess ? OK : ERR_HIP;
    if (e) set_error("window_attention_ws: bias upload failed");
    else e = launch_win_attn14((const bf16_t*)qkv, (const float*)d, (bf16_t*)out, B, res, C, heads, st);
    if (hipStreamSynchronize(st) != hipSuccess && !e) {
        set_error("window_attention_ws: stream synchronisation failed");
        e = ERR_HIP;
    }
    MI355_CHECK_HIP(hipFree(d));
    return e;
}

extern "C" int mi355_swin_layernorm(const void* in, const float* gamma, const float* beta, void* out, int64_t rows, int C, int merge, int gh,
                                    int gw, int stats, float eps, void* stream) {
    using namespace mi355;
    MI355_REQUIRE(in && out && (stats || (gamma && beta)), "swin_layernorm: null pointer");
    MI355_REQUIRE((merge == 0 || merge == 1) && (stats == 0 || stats == 1), "swin_layernorm: merge and stats are 0 or 1");
    MI355_REQUIRE(!(merge && stats), "swin_layernorm: merge with stats is not instantiated");
    bool width_ok = false;
    for (int c : {96, 192, 384, 768, 1536, 128, 256, 512, 1024, 2048}) width_ok |= c == C;
    MI355_REQUIRE(width_ok, "swin_layernorm: unsupported width %d", C);
    MI355_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31), "swin_layernorm: bad shape rows=%lld", (long long)rows);
    if (merge) {
        MI355_REQUIRE(gh >= 1 && gw >= 1 && gh <= 16384 && gw <= 16384, "swin_layernorm: bad shape gh=%d gw=%d", gh, gw);
        MI355_REQUIRE(rows % ((int64_t)gh * gw) == 0, "swin_layernorm: rows=%lld must be a multiple of gh * gw = %d", (long long)rows,
                      gh * gw);
    }
    MI355_REQUIRE(eps > 0.f && eps < 1.f, "swin_layernorm: eps %g out of range", (double)eps);
    MI355_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)gamma % 16 == 0 && (uintptr_t)beta % 16 == 0,
                  "swin_layernorm: pointers must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const bf16_t* i = (const bf16_t*)in;
    bf16_t* o = (bf16_t*)out;
    if (stats) return launch_ln<false, true>(i, nullptr, nullptr, o, rows, C, 0, 0, eps, st);
    if (merge) return launch_ln<true>(i, gamma, beta, o, rows, C, gh, gw, eps, st);
    return launch_ln<false>(i, gamma, beta, o, rows, C, 0, 0, eps, st);
}

extern "C" int mi355_swin_patch_embed(const float* x, const unsigned char* images, const int64_t* desc_dev, int b0, int B, int H, int h, int w,
                                      int fill, const float* mean, const float* stdv, const float* weight, const float* bias,
                                      const float* gamma, const float* beta, int embed, float eps, void* out, void* stream) {
    using namespace mi355;
    MI355_REQUIRE(!x != !images, "swin_patch_embed: exactly one of x and images");
    MI355_REQUIRE(weight && bias && gamma && beta && out, "swin_patch_embed: null pointer");
    MI355_REQUIRE(embed == 128 || embed == 96, "swin_patch_embed: embed %d (128 or 96)", embed);
    MI355_REQUIRE(B >= 1 && B <= 65535, "swin_patch_embed: bad shape B=%d", B);
    MI355_REQUIRE(eps > 0.f && eps < 1.f, "swin_patch_embed: eps %g out of range", (double)eps);
    if (x) {
        MI355_REQUIRE(!desc_dev, "swin_patch_embed: desc_dev goes with images");
        MI355_REQUIRE(H >= 4 && H <= 224 && H % 4 == 0, "swin_patch_embed: H=%d must be a multiple of 4 in [4, 224]", H);
    } else {
        MI355_REQUIRE(H == 224, "swin_patch_embed: uint8 images fill the 224 x 224 square (H=%d)", H);
        MI355_REQUIRE(mean && stdv, "swin_patch_embed: null pointer (mean, stdv)");
        MI355_REQUIRE(fill >= 0 && fill <= 255, "swin_patch_embed: fill %d out of range", fill);
        if (desc_dev) MI355_REQUIRE(b0 >= 0, "swin_patch_embed: b0=%d is negative", b0);
        else MI355_REQUIRE(h >= 1 && w >= 1 && std::max(h, w) == 224, "swin_patch_embed: longer side must be 224 (got %dx%d)", h, w);
    }
    MI355_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)bias % 16 == 0 && (uintptr_t)gamma % 16 == 0 &&
                      (uintptr_t)beta % 16 == 0 && (uintptr_t)weight % 4 == 0 && (uintptr_t)desc_dev % 8 == 0,
                  "swin_patch_embed: x, bias, gamma, beta and out must be 16-byte aligned (weight 4, desc_dev 8)");
    const hipStream_t st = (hipStream_t)stream;
    std::vector<float> wt((size_t)embed * 48), packed((size_t)embed * 48);
    std::vector<int64_t> desc(images && desc_dev ? (size_t)B * 3 : 0);
    MI355_CHECK_HIP(hipMemcpyAsync(wt.data(), weight, wt.size() * 4, hipMemcpyDeviceToHost, st));
    if (!desc.empty()) MI355_CHECK_HIP(hipMemcpyAsync(desc.data(), desc_dev + (size_t)b0 * 3, desc.size() * 8, hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    for (size_t b = 0; b < desc.size() / 3; ++b)    // the ragged sizes live on the device: the same rule, after the copy
        MI355_REQUIRE(desc[3 * b] >= 0 && desc[3 * b + 1] >= 1 && desc[3 * b + 2] >= 1 && std::max(desc[3 * b + 1], desc[3 * b + 2]) == 224,
                      "swin_patch_embed: longer side must be 224 (image %d is %lldx%lld)", b0 + (int)b, (long long)desc[3 * b + 1],
                      (long long)desc[3 * b + 2]);
    swin_patch_weight(wt.data(), embed, packed.data());
    PatchU8RaggedArgs r{};
    if (images) r = patch_u8_args(images, h, w, fill, mean, stdv, desc_dev, b0);
    void* d = nullptr;
    MI355_CHECK_HIP(hipMalloc(&d, packed.size() * 4));
    int e = hipMemcpyAsync(d, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess ? OK : ERR_HIP;
    if (e) set_error("swin_patch_embed: weight upload failed");
    else e = launch_patch_embed(x, r, embed, (const float*)d, bias, gamma, beta, (bf16_t*)out, B, H, 224, eps, st);
    if (hipStreamSynchronize(st) != hipSuccess && !e) {
        set_error("swin_patch_embed: stream synchronisation failed");
        e = ERR_HIP;
    }
    MI355_CHECK_HIP(hipFree(d));
    return e;
}

extern "C" int mi355_swin_ln_token_mean(const void* in, const float* gamma, const float* beta, float* pooled, void* pooled_bf16, int B, int L,
                                        int C, float eps, void* stream) {
    using namespace mi355;
    MI355_REQUIRE(in && gamma && beta && pooled && pooled_bf16, "swin_ln_token_mean: null pointer");
    MI355_REQUIRE(C == 1024 || C == 768, "swin_ln_token_mean: unsupported width %d (1024 or 768)", C);
    MI355_REQUIRE(B >= 1 && L >= 1, "swin_ln_token_mean: bad shape B=%d L=%d", B, L);
    MI355_REQUIRE((size_t)B * L * C < ((size_t)1 << 40), "swin_ln_token_mean: tensor too large");
    MI355_REQUIRE(eps > 0.f && eps < 1.f, "swin_ln_token_mean: eps %g out of range", (double)eps);
    MI355_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)gamma % 4 == 0 && (uintptr_t)beta % 4 == 0 && (uintptr_t)pooled % 4 == 0 &&
                      (uintptr_t)pooled_bf16 % 2 == 0,
                  "swin_ln_token_mean: in must be 16-byte aligned (gamma, beta, pooled 4, pooled_bf16 2)");
    return launch_ln_token_mean((const bf16_t*)in, gamma, beta, pooled, (bf16_t*)pooled_bf16, B, L, C, eps, (hipStream_t)stream);
}
