// Body of k_cos_gemm and k_cos_gemm_filt (rank.hip): included into both, so the unfiltered kernel compiles from exactly
// the text it always had.  FILT (constexpr bool) and flt (RankFilter) are declared by the including kernel.
    // x0 / ntx: this launch covers the column tiles [x0, x0 + xtiles) of ntx for ny query blocks (the host splits a call into a main launch
    // of whole rounds and a tail launch of smaller tiles)
    constexpr int BM = 64 * MT;
    constexpr int RK_LD = RK_BK + 4;      // +4 floats: ds_read_b128 of 16 distinct rows is bank-conflict free (36 and 20)
    constexpr int CPR = RK_BK / 4;        // float4 columns per row of a K-tile
    constexpr int RPP = 256 / CPR;        // rows covered by one pass of the 256 threads
    constexpr int A_LOADS = BM / RPP;     // float4 loads per thread per K-tile for A
    constexpr int B_LOADS = RK_BN / RPP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [2][BM][RK_LD]
    float* Bs = smem + 2 * BM * RK_LD;         // [2][RK_BN][RK_LD]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by;
    rank_tile_of((int)blockIdx.x, xtiles, ny, bx, by);
    const i64 n0 = (i64)(bx + x0) * RK_BN;
    const int m0 = by * BM;

    const int c4 = tid % CPR;  // float4 column within the K-tile
    const int r0 = tid / CPR;

    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4 ra[A_LOADS], rb[B_LOADS];

    auto load_tile = [&](int k0) {
        const int k = k0 + c4 * 4;
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const int row = m0 + r0 + RPP * i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < Q) {
                const float* p = Qn + (i64)row * D + k;
                if (VEC) {
                    if (k + 3 < D) v = *reinterpret_cast<const f32x4*>(p);
                } else {
                    if (k + 0 < D) v.x = p[0];
                    if (k + 1 < D) v.y = p[1];
                    if (k + 2 < D) v.z = p[2];
                    if (k + 3 < D) v.w = p[3];
                }
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const i64 row = n0 + r0 + RPP * i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < G) {
                const float* p = Gal + row * D + k;
                if (VEC) {
                    if (k + 3 < D) v = *reinterpret_cast<const f32x4*>(p);
                } else {
                    if (k + 0 < D) v.x = p[0];
                    if (k + 1 < D) v.y = p[1];
                    if (k + 2 < D) v.z = p[2];
                    if (k + 3 < D) v.w = p[3];
                }
            }
            rb[i] = v;
        }
    };
    auto store_tile = [&](int buf) {
        float* a = As + buf * BM * RK_LD;
        float* b = Bs + buf * RK_BN * RK_LD;
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i)
            *reinterpret_cast<f32x4*>(a + (r0 + RPP * i) * RK_LD + c4 * 4) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i)
            *reinterpret_cast<f32x4*>(b + (r0 + RPP * i) * RK_LD + c4 * 4) = rb[i];
    };

    const int nt = (D + RK_BK - 1) / RK_BK;
    load_tile(0);
    store_tile(0);
    __syncthreads();

    const int lr = lane & 31;
    const int lk = (lane >> 5) * 4;
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) load_tile((t + 1) * RK_BK);
        const float* a = As + buf * BM * RK_LD + (wm * MT * 32 + lr) * RK_LD + lk;
        const float* b = Bs + buf * RK_BN * RK_LD + (wn * 64 + lr) * RK_LD + lk;
#pragma unroll
        for (int t8 = 0; t8 < RK_BK / 8; ++t8) {
            f32x4 af[MT], bfr[2];
#pragma unroll
            for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const f32x4*>(a + i * 32 * RK_LD + t8 * 8);
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = *reinterpret_cast<const f32x4*>(b + j * 32 * RK_LD + t8 * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bfr[j][e], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nt) store_tile(buf ^ 1);
        __syncthreads();
    }

    cos_gemm_epilogue<MT, FK, FILT>(acc, smem, ginv, S, Q, G, k, cand_val, cand_idx, x0, ntx, n0, m0, flt);
