// Body of k_topk_small and k_topk_small_filt (rank.hip): included into both, so the unfiltered kernel compiles from exactly
// the text it always had.  FILT (constexpr bool) and flt (RankFilter) are declared by the including kernel.
// TOPK_SMALL_VALUE(j): the score of candidate j; the PQ scan (pq.hip) defines it as the table lookup of row j, so that its
// scores never exist in memory.
// TOPK_SMALL_THREADS: the threads of the including kernel's workgroup (a multiple of 64).
// TOPK_SMALL_ROW(j): the gallery row of candidate j, which its implicit index, its label and the excluded row go by; the IVF-PQ
// scan (ivfpq.hip) visits rows in list order and defines it as the list's entry for position j (evaluated after the value).
// TOPK_SMALL_SKIP(j): true for a position that holds no candidate (there: a list entry outside the gallery).
#ifndef TOPK_SMALL_VALUE
#define TOPK_SMALL_VALUE(j) v[j]
#endif
#ifndef TOPK_SMALL_THREADS
#define TOPK_SMALL_THREADS 256
#endif
#ifndef TOPK_SMALL_ROW
#define TOPK_SMALL_ROW(j) (j)
#endif
#ifndef TOPK_SMALL_SKIP
#define TOPK_SMALL_SKIP(j) false
#endif
    const int tid = threadIdx.x;
    const i64 q = blockIdx.y;
    const i64 c0 = (i64)blockIdx.x * chunk_len;
    const i64 c1 = min(rowlen, c0 + chunk_len);
    const float* v = vals + q * in_stride;
    const i64* ix = idxs ? idxs + q * in_stride : nullptr;
    const int* ix32 = idxs32 ? idxs32 + q * in_stride : nullptr;

    float lv[K];
    i64 li[K];
#pragma unroll
    for (int i = 0; i < K; ++i) { lv[i] = NEG_INF; li[i] = IDX_PAD; }
    i64 fq_lab = 0, fq_ex = -1;
    if constexpr (FILT) query_filter(flt, q, fq_lab, fq_ex);

    for (i64 j = c0 + tid; j < c1; j += TOPK_SMALL_THREADS) {
        const float x = TOPK_SMALL_VALUE(j);
        i64 id;
        if (ix32) { const int t = ix32[j]; id = t == IDX32_PAD ? IDX_PAD : (i64)t + idx_offset; }
        else id = ix ? ix[j] : TOPK_SMALL_ROW(j) + idx_offset;
        if constexpr (FILT) {
            if (!eligible(flt.mode, fq_lab, flt.mode != MI355_LABEL_ANY ? flt.glab[TOPK_SMALL_ROW(j)] : 0, fq_ex, TOPK_SMALL_ROW(j)))
                id = IDX_PAD;
        }
        if (TOPK_SMALL_SKIP(j)) id = IDX_PAD;
        if (id < NO_CAND_IDX && better(x, id, lv[K - 1], li[K - 1])) {      // (IDX_PAD and the shard pad: no candidate)
            lv[K - 1] = x; li[K - 1] = id;
#pragma unroll
            for (int i = K - 1; i > 0; --i) {
                if (better(lv[i], li[i], lv[i - 1], li[i - 1])) {
                    float tv = lv[i]; lv[i] = lv[i - 1]; lv[i - 1] = tv;
                    i64 ti = li[i]; li[i] = li[i - 1]; li[i - 1] = ti;
                }
            }
        }
    }

    __shared__ float sv[TOPK_SMALL_THREADS / 64];
    __shared__ i64 si[TOPK_SMALL_THREADS / 64];
    const int lane = tid & 63, wave = tid >> 6;
    float* o_v = ov + (q * gridDim.x + blockIdx.x) * k;
    i64* o_i = oi + (q * gridDim.x + blockIdx.x) * k;
    for (int r = 0; r < k; ++r) {
        float bv = lv[0];
        i64 bi = li[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov2 = __shfl_xor(bv, o, 64);
            const i64 oi2 = __shfl_xor(bi, o, 64);
            if (better(ov2, oi2, bv, bi)) { bv = ov2; bi = oi2; }
        }
        if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
#pragma unroll
        for (int w = 1; w < TOPK_SMALL_THREADS / 64; ++w)
            if (better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        if (tid == 0) { o_v[r] = bv; o_i[r] = bi; }
        // the owner pops its head (indices are unique among real entries; pads never win a real slot)
        if (li[0] == bi && bi != IDX_PAD) {      // (by index only: a NaN score does not compare equal to itself)
#pragma unroll
            for (int i = 0; i < K - 1; ++i) { lv[i] = lv[i + 1]; li[i] = li[i + 1]; }
            lv[K - 1] = NEG_INF; li[K - 1] = IDX_PAD;
        }
        __syncthreads();
    }
