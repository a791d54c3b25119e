// Body of k_cos_gemm_f16 and k_cos_gemm_f16_filt (rank_f16.hip): included into both, so the unfiltered kernel compiles from exactly
// the text it always had.  FILT (constexpr bool) and flt (RankFilter) are declared by the including kernel.
    constexpr int BM = 64 * MT;
    constexpr int A_PIECES = (BM / 32) * 8;           // 1 KB pieces per stage: 4 sub-steps x 2 planes per row block
    constexpr int A_STAGE = A_PIECES * 512;           // f16 elements per stage
    constexpr int B_STAGE = RK_BN * F16_KSTEP;        // f16 elements per stage (16 KB)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f16* As = reinterpret_cast<f16*>(smem);           // [2][BM/32][4][2][512]
    f16* Bs = As + 2 * A_STAGE;                       // [3][128][64], chunks swizzled

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31;
    int bx, by;
    rank_tile_of((int)blockIdx.x, xtiles, ny, bx, by);
    const i64 n0 = (i64)(bx + x0) * RK_BN;
    const int m0 = by * BM;
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    const int n_steps = ld / F16_KSTEP, n_sub = ld / 16;

    // B: wave w moves pieces 4w .. 4w + 3; lane -> row 8 * piece + lane / 8, LDS position lane % 8
    const f16* b_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (swave * 4 + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        const i64 g = n0 + r < G ? n0 + r : G - 1;
        b_src[i] = Gal + g * ld + c * 8;
    }
    // (k-steps past the end re-read the last one: the data is never used, the count of pieces in flight stays uniform)
    auto dma_b = [&](int stage, int t) {
        const int tt = t < n_steps ? t : n_steps - 1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            glds16(reinterpret_cast<const bf16_t*>(b_src[i] + tt * F16_KSTEP),
                   reinterpret_cast<bf16_t*>(Bs + stage * B_STAGE + (swave * 4 + i) * 512));
    };
    // A: piece p = (row block p / 8, sub-step (p % 8) / 2, plane p % 2) of k-step t sits at
    // Qs + ((m0/32 + p/8) * n_sub + 4t) * 1024 + (p % 8) * 512; wave w moves pieces w, w + 4, ...
    const f16* a_src[A_PIECES / 4];
#pragma unroll
    for (int i = 0; i < A_PIECES / 4; ++i) {
        const int p = swave + 4 * i;
        a_src[i] = Qs + ((size_t)(m0 / 32 + p / 8) * n_sub) * 1024 + (p % 8) * 512 + lane * 8;
    }
    auto dma_a = [&](int buf, int t) {
#pragma unroll
        for (int i = 0; i < A_PIECES / 4; ++i)
            glds16(reinterpret_cast<const bf16_t*>(a_src[i] + (size_t)t * 4 * 1024),
                   reinterpret_cast<bf16_t*>(As + buf * A_STAGE + (swave + 4 * i) * 512));
    };

    f32x16 acc[MT][2], acc_lo[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; acc_lo[i][j][e] = 0.f; }

    // B fragment reads: row r = wn * 64 + j * 32 + lr, chunk 2s + (lane >> 5) of sub-step s at its swizzled position
    int b_off[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = wn * 64 + j * 32 + lr;
#pragma unroll
        for (int s = 0; s < 4; ++s) b_off[j][s] = r * F16_KSTEP + (((2 * s + (lane >> 5)) ^ ((r >> 1) & 7)) << 3);
    }
    auto compute = [&](int abuf, int bstage) {
        const f16* a = As + abuf * A_STAGE + (wm * MT) * 8 * 512 + lane * 8;
        const f16* b = Bs + bstage * B_STAGE;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            f16x8 bf[2], ah[MT], al[MT];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const f16x8*>(b + b_off[j][s]);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                ah[i] = *reinterpret_cast<const f16x8*>(a + (i * 8 + s * 2) * 512);
                al[i] = *reinterpret_cast<const f16x8*>(a + (i * 8 + s * 2 + 1) * 512);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc_lo[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bf[j], acc_lo[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bf[j], acc[i][j], 0, 0, 0);
                }
        }
    };

    dma_a(0, 0);
    dma_b(0, 0);
    dma_b(1, 1);
    __syncthreads();                   // drains vmcnt: everything has landed

    int bs_cur = 0, bs_far = 2;        // B stage of k-step t / of k-step t + 2
    for (int t = 0; t < n_steps; ++t) {
        if (t + 1 < n_steps) dma_a((t & 1) ^ 1, t + 1);   // everybody left this buffer at the previous barrier
        __builtin_amdgcn_sched_barrier(0);                // (the count below needs the A pieces issued BEFORE the B pieces)
        dma_b(bs_far, t + 2);
        __builtin_amdgcn_sched_barrier(0);
        compute(t & 1, bs_cur);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); // A(t+1) and B(t+1) have landed; the four B(t+2) pieces stay in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        bs_cur = bs_cur == 2 ? 0 : bs_cur + 1;
        bs_far = bs_far == 2 ? 0 : bs_far + 1;
    }
    __syncthreads();                   // the last look-ahead pieces have landed before the epilogue reuses the LDS
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = __builtin_fmaf(acc_lo[i][j][e], F16_LO_UNSCALE, acc[i][j][e]);
    cos_gemm_epilogue<MT, FK, FILT>(acc, smem, nullptr, S, Q, G, k, cand_val, cand_idx, x0, ntx, n0, m0, flt);
