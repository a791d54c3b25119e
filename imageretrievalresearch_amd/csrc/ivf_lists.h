// What the scans of probed lists share (ivf.hip: fp32 / fp16 rows read in place; ivfpq.hip: a list-ordered copy of PQ codes): the
// bounds of a list in the lists' CSR and the words their kernels raise for bad device-side data.  gfx950 only.
#pragma once
#include "rank_common.h"

namespace mi355 {

constexpr i64 IVF_MAX_WGS = ((i64)1 << 24) - 1;
enum { IVF_FLAG_ENTRY = 0, IVF_FLAG_CAP = 1, IVF_FLAGS = 2 };

// The rows [b, e) of list l in order; false (and an empty range) when the offsets do not ascend within [0, G]
__device__ __forceinline__ bool list_range(const i64* __restrict__ offsets, i64 l, i64 G, i64& b, i64& e) {
    b = offsets[l];
    e = offsets[l + 1];
    if (b >= 0 && b <= e && e <= G) return true;
    e = b = 0;
    return false;
}

}  // namespace mi355
