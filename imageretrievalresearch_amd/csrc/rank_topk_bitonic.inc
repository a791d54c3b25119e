// Body of k_topk_bitonic and k_topk_bitonic_filt (rank.hip): included into both, so the unfiltered kernel compiles from exactly
// the text it always had.  FILT (constexpr bool) and flt (RankFilter) are declared by the including kernel.
    __shared__ float sv[BT_N];
    __shared__ i64 si[BT_N];
    const int tid = threadIdx.x;
    const i64 q = blockIdx.y;
    const i64 c0 = (i64)blockIdx.x * BT_N;
    const float* v = vals + q * in_stride;
    const i64* ix = idxs ? idxs + q * in_stride : nullptr;
    i64 fq_lab = 0, fq_ex = -1;
    if constexpr (FILT) query_filter(flt, q, fq_lab, fq_ex);
    for (int j = tid; j < BT_N; j += 256) {
        const i64 g = c0 + j;
        if (g < rowlen) {
            sv[j] = v[g];
            si[j] = ix ? ix[g] : g + idx_offset;
            if (si[j] >= NO_CAND_IDX) { sv[j] = NEG_INF; si[j] = IDX_PAD; }      // explicit "no candidate": whatever its value
            if constexpr (FILT) {
                if (!eligible(flt.mode, fq_lab, flt.mode != MI355_LABEL_ANY ? flt.glab[g] : 0, fq_ex, g)) {
                    sv[j] = NEG_INF;
                    si[j] = IDX_PAD;
                }
            }
        } else {
            sv[j] = NEG_INF;
            si[j] = IDX_PAD;
        }
    }
    __syncthreads();
    for (int size = 2; size <= BT_N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < BT_N / 2; t += 256) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);  // first half of each size-block sorted descending
                const float a = sv[lo], b = sv[hi];
                const i64 ia = si[lo], ib = si[hi];
                const bool swap = desc ? better(b, ib, a, ia) : better(a, ia, b, ib);
                if (swap) { sv[lo] = b; sv[hi] = a; si[lo] = ib; si[hi] = ia; }
            }
            __syncthreads();
        }
    }
    float* o_v = ov + (q * gridDim.x + blockIdx.x) * k;
    i64* o_i = oi + (q * gridDim.x + blockIdx.x) * k;
    for (int j = tid; j < k; j += 256) { o_v[j] = sv[j]; o_i[j] = si[j]; }
