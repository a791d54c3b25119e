// Body of k_cos_gemm_split and k_cos_gemm_split_filt (rank.hip): included into both, so the unfiltered kernel compiles from exactly
// the text it always had.  FILT (constexpr bool) and flt (RankFilter) are declared by the including kernel.
    constexpr int BM = 64 * MT;
    constexpr int BK = 16;
    constexpr int A_STAGE = (BM / 32) * 3 * 512;      // bf16 elements per stage
    constexpr int A_PIECES = (BM / 32) * 3;           // 1 KB pieces per stage
    constexpr int B_STAGE = RK_BN * BK;               // floats per stage (8 KB)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    bf16_t* As = reinterpret_cast<bf16_t*>(smem);                       // [A_RING][BM/32][3][512]
    // A ring: 2 stages at MT = 2 (the pieces come from L2 one k-step ahead; a third stage would cost the third workgroup per
    // CU), 3 stages at MT = 1 (two k-steps ahead: the 64-row tiles are the tail launch and the small-Q shapes, few
    // workgroups per CU with nothing else to hide a piece's latency behind)
    constexpr int A_RING = MT == 1 ? 3 : 2;
    float* Bs = smem + (A_RING * A_STAGE * 2) / 4;                      // [3][128][16], chunks swizzled

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by;
    rank_tile_of((int)blockIdx.x, xtiles, ny, bx, by);
    const i64 n0 = (i64)(bx + x0) * RK_BN;
    const int m0 = by * BM;
    // the wave index as a scalar: piece selection becomes scalar branches (a per-lane branch around a load makes hipcc
    // drain vmcnt)
    const int swave = __builtin_amdgcn_readfirstlane(wave);

    // B: wave w moves pieces 2w and 2w + 1 (rows 32w .. 32w + 31); lane -> row 16 * piece + lane / 4, position lane % 4
    const float* b_row[2];
    int b_k[2];
    bool b_ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (swave * 2 + i) * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 2) & 3);
        b_ok[i] = n0 + r < G;
        b_row[i] = Gal + (b_ok[i] ? (n0 + r) * D : 0);
        b_k[i] = c * 4;
    }
    auto dma_b = [&](int stage, int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ok = b_ok[i] && k0 + b_k[i] < D;                // D % 4 == 0: a chunk is inside or outside
            glds16(reinterpret_cast<const bf16_t*>(ok ? b_row[i] + k0 + b_k[i] : zeros),
                   reinterpret_cast<bf16_t*>(Bs + stage * B_STAGE + (swave * 2 + i) * 256));
        }
    };
    // A: piece (row block rbl, plane p) of k-step t sits at Qs + (((m0/32 + rbl) * n_steps + t) * 3 + p) * 512.
    // 12 (MT = 2) or 6 (MT = 1) pieces per stage: wave w moves pieces w, w + 4, w + 8 / pieces w and (w < 2) w + 4.
    const bf16_t* a_src = Qs + (size_t)(m0 / 32) * n_steps * 3 * 512 + lane * 8;
    const bf16_t* a_piece[(A_PIECES + 3) / 4];
#pragma unroll
    for (int i = 0; i < (A_PIECES + 3) / 4; ++i) {
        const int piece = (swave + 4 * i) % A_PIECES;
        a_piece[i] = a_src + ((size_t)((piece / 3) * n_steps) * 3 + piece % 3) * 512;
    }
    auto dma_a = [&](int buf, int t) {
#pragma unroll
        for (int i = 0; i < (A_PIECES + 3) / 4; ++i) {
            const int piece = swave + 4 * i;
            if (A_PIECES % 4 == 0 || i < A_PIECES / 4 || swave < A_PIECES % 4)
                glds16(a_piece[i] + (size_t)t * 3 * 512, As + buf * A_STAGE + piece * 512);
        }
    };

    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int lr = lane & 31;
    // B fragment reads: row r = wn * 64 + j * 32 + lr, chunks 2 * (lane >> 5) and + 1 at their swizzled positions
    int b_off[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = wn * 64 + j * 32 + lr, sw = (r >> 2) & 3, c0 = (lane >> 5) * 2;
        b_off[j][0] = r * BK + ((c0 ^ sw) << 2);
        b_off[j][1] = r * BK + (((c0 + 1) ^ sw) << 2);
    }
    auto compute = [&](int abuf, int bstage) {
        const bf16_t* a = As + abuf * A_STAGE + (wm * MT * 3) * 512 + lane * 8;
        const float* b = Bs + bstage * B_STAGE;
        bf16x8 af[MT][3];
        u32x4 bh[2], bm[2], bl[2];
        f32x4 v0[2], v1[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            v0[j] = *reinterpret_cast<const f32x4*>(b + b_off[j][0]);
            v1[j] = *reinterpret_cast<const f32x4*>(b + b_off[j][1]);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int p = 0; p < 3; ++p) af[i][p] = *reinterpret_cast<const bf16x8*>(a + (i * 3 + p) * 512);
        split3(v0[0], v1[0], bh[0], bm[0], bl[0]);
        // Per fragment j: six products for each of the MT row blocks, smallest terms first (the order is the same for every
        // (query, gallery row) pair wherever its tile lies).  The split of fragment 1 is issued in the gaps of fragment 0's
        // MFMAs (an MFMA holds the vector issue for 8 of its 32 cycles): sched_group_barrier pins "1 MFMA, 4 VALU" groups.
        auto products = [&](int j) {
            const bf16x8 gh = *reinterpret_cast<const bf16x8*>(&bh[j]);
            const bf16x8 gm = *reinterpret_cast<const bf16x8*>(&bm[j]);
            const bf16x8 gl = *reinterpret_cast<const bf16x8*>(&bl[j]);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][2], gh, acc[i][j], 0, 0, 0);   // l * h'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], gl, acc[i][j], 0, 0, 0);   // h * l'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], gm, acc[i][j], 0, 0, 0);   // m * m'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][1], gh, acc[i][j], 0, 0, 0);   // m * h'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], gm, acc[i][j], 0, 0, 0);   // h * m'
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][0], gh, acc[i][j], 0, 0, 0);   // h * h'
            }
        };
        split3(v0[1], v1[1], bh[1], bm[1], bl[1]);
        products(0);
#pragma unroll
        for (int g = 0; g < 6 * MT; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);   // four VALU (of fragment 1's split)
        }
        products(1);
    };

    dma_a(0, 0);
    if (A_RING == 3 && n_steps > 1) dma_a(1, 1);
    dma_b(0, 0);
    dma_b(1, BK);                      // (zeros past D)
    __syncthreads();                   // drains vmcnt: everything has landed

    int bs_cur = 0, bs_far = 2;        // B stage of k-step t / of k-step t + 2 (and, at A_RING == 3, the A stages)
    for (int t = 0; t < n_steps; ++t) {
        if constexpr (A_RING == 2) {
            if (t + 1 < n_steps) dma_a((t & 1) ^ 1, t + 1);  // everybody left these buffers at the previous barrier
        } else {
            if (t + 2 < n_steps) dma_a(bs_far, t + 2);
        }
        __builtin_amdgcn_sched_barrier(0);                   // (the counts below need the A pieces issued BEFORE the B pieces)
        dma_b(bs_far, (t + 2) * BK);
        __builtin_amdgcn_sched_barrier(0);
        compute(A_RING == 2 ? (t & 1) : bs_cur, bs_cur);
        if constexpr (A_RING == 2) {
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); // A(t+1) and B(t+1) have landed; B(t+2) stays in flight
        } else {
            // A(t+2) (two pieces from waves 0 and 1, one from waves 2 and 3; none at the end) and B(t+2) stay in flight
            if (t + 2 >= n_steps) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else if (swave < A_PIECES % 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        bs_cur = bs_cur == 2 ? 0 : bs_cur + 1;
        bs_far = bs_far == 2 ? 0 : bs_far + 1;
    }
    __syncthreads();                   // the last look-ahead pieces (zeros) have landed before the epilogue reuses the LDS
    cos_gemm_epilogue<MT, FK, FILT>(acc, smem, ginv, S, Q, G, k, cand_val, cand_idx, x0, ntx, n0, m0, flt);
