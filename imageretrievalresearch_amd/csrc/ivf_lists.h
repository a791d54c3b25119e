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

// The part of a scan's shape that both entries bound alike: at least one query, 1 <= nprobe <= nlist < 2^24, Q * nprobe < 2^31
// pairs and Q * cap <= 2^40 candidate slots
static inline bool ivf_lists_shape_ok(i64 Q, int nprobe, i64 nlist, i64 cap) {
    return Q >= 1 && nlist >= 1 && nlist <= IVF_MAX_WGS && nprobe >= 1 && nprobe <= nlist && cap >= 1 &&
           Q <= (((i64)1 << 31) - 1) / nprobe && cap <= ((i64)1 << 40) / Q;
}

// The end of both entries: the words `flag` [IVF_FLAGS] that the kernels raised - and, where there is one, the word of
// members_async over the probes - read back behind one stream sync; bad lists are refused.
static inline int ivf_check_flags(const unsigned* flag, const unsigned* members_flag, i64 nlist, i64 G, i64 cap, const char* who,
                                  hipStream_t st) {
    unsigned flags[IVF_FLAGS] = {0, 0}, bad_probe = 0;
    MI355_CHECK_HIP(hipMemcpyAsync(flags, flag, sizeof(flags), hipMemcpyDeviceToHost, st));
    if (members_flag) MI355_CHECK_HIP(hipMemcpyAsync(&bad_probe, members_flag, sizeof(bad_probe), hipMemcpyDeviceToHost, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));
    MI355_REQUIRE(!bad_probe && !flags[IVF_FLAG_ENTRY], "%s: a list id outside [0, nlist=%lld), an order entry outside [0, G=%lld) "
                  "or offsets that do not ascend within [0, G]", who, (long long)nlist, (long long)G);
    MI355_REQUIRE(!flags[IVF_FLAG_CAP], "%s: a query's probed lists hold more than cap=%lld rows", who, (long long)cap);
    return OK;
}

}  // namespace mi355
