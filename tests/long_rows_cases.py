"""The inputs and the modelled bugs of the long-row tests (test_long_rows_gpu.py on the GPU, test_long_rows_args.py without
one): rows so long that the row walkers take a second trip of their 4 x 64-unit loop, and dims on either side of every step
of the IVF scan's group size (over fp32, fp16 and int8 rows).  NumPy only.

The constants below are restated from the kernels they aim at: row_dot.h and k_cos_gemv_f16 walk 4 x 64 units of 8 halves
(2048 elements) per trip, row_dot's fp32 branch 4 x 64 units of 4 floats (1024), k_cos_gemv_i8 4 x 64 units of 16 codes (4096).
Seeded Gaussian rows whose elements past the first trip are multiplied by 8 before anything normalises them, so that the tail
carries a visible share of every score: a walker that drops, repeats or misplaces it misses by far more than SCORE_TOL."""
import numpy as np

import ivf_ref

FIRST_TRIP = {"f16": 2048, "f32": 1024, "i8": 4096}
UNIT = {"f16": 8, "f32": 4}                                          # elements of one lane's load (row_dot.h)
TAIL_GAIN = 8.0

# mi355_rescore_candidates: the end of the first trip, one unit past it (fp32: one unit, then scalar lanes), several trips, and
# the longest query the 64 KB of LDS hold
RESCORE_DIMS = {"f16": [2048, 2056, 4096, 16384], "f32": [1024, 1028, 4099, 16384]}
RESCORE_G, RESCORE_Q = 200, 5
TOO_LONG = 16388                                                     # ldq * 4 bytes > 64 KB for either dtype

# IVF scan: the group of ivf_group() is min(4, 64 KB / (ldq * 4)) queries - both sides of 4 -> 3, 3 -> 2, 2 -> 1, and the end
IVF_DIMS = {"f32": [4096, 4099, 5460, 5464, 8192, 8196, 16384], "f16": [4096, 4104, 5456, 5464, 8192, 8200, 16384]}
IVF_NQ = {4096: 4, 4099: 3, 4104: 3, 5456: 3, 5460: 3, 5464: 2, 8192: 2, 8196: 1, 8200: 1, 16384: 1}
IVF_LENGTHS = [64, 0, 1, 65, 70]                                     # five hand-made lists over 200 rows, one of them empty
IVF_G, IVF_Q = sum(IVF_LENGTHS), 9
IVF_PROBES = [3, 1, 4, 0, 2]                                         # every query probes every list in this order

# IVF scan over int8 rows: a query is two int8 planes of lq = dim rounded up to 128 bytes, the group of ivf_group_i8() is
# min(8, 64 KB / (2 * lq)) queries - 8, then both sides of 8 -> 7 ... and 2 -> 1, and the one query that fills the 64 KB alone
I8_SEGMENT, IVF_LDS, IVF_MAXQ_I8 = 128, 64 * 1024, 8
IVF_DIMS_I8 = [4096, 4100, 8192, 8200, 16384, 16400, 32768]
IVF_GROUP_I8 = {4096: 8, 4100: 7, 8192: 4, 8200: 3, 16384: 2, 16400: 1, 32768: 1}
IVF_SPLIT_I8 = {8: [8, 1], 7: [7, 2], 4: [4, 4, 1], 3: [3, 3, 3], 2: [2, 2, 2, 2, 1], 1: [1] * 9}         # of the 9 queries of one list

# The GEMVs behind search(q[:Q], k): (D, Q) -> whether the LDS rule lets the GEMV run
GEMV_G = 1000
GEMV_F16 = {(D, Q): Q * D * 4 <= 64 * 1024 for D in (2048, 2112, 4096, 4160) for Q in (1, 2, 3, 4)}      # D = ld (a multiple of 64)
GEMV_F32 = {(3840, 4): True, (3844, 4): False, (15360, 1): True}                                          # Q * D * 4 <= 60 KB
GEMV_I8 = {(D, Q): Q * 2 * D <= 64 * 1024 for D in (4096, 4224, 8192, 8320) for Q in (1, 4)}              # D = ld (a multiple of 128)


def ldq(D, kind):
    """Floats of one query in LDS: dim rounded up to a unit (row_dot_ldq)."""
    u = UNIT[kind]
    return (D + u - 1) // u * u


def ivf_nq(D, kind):
    """Queries of one group of the IVF scan (ivf_group): 0 when not even one fits."""
    return min(4, (64 * 1024) // (ldq(D, kind) * 4))


def lq_i8(D):
    """Bytes of one int8 plane of a query in LDS: dim rounded up to a 128-byte segment (i8_ld)."""
    return (D + I8_SEGMENT - 1) // I8_SEGMENT * I8_SEGMENT


def ivf_nq_i8(D):
    """Queries of one group of the IVF scan over int8 rows (ivf_group_i8): 0 when not even one fits."""
    return min(IVF_MAXQ_I8, IVF_LDS // (2 * lq_i8(D)))


def raw(kind, seed, n, D):
    """(n, D) float32: seeded Gaussian rows, the elements past the kind's first trip multiplied by TAIL_GAIN."""
    x = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    x[:, FIRST_TRIP[kind]:] *= np.float32(TAIL_GAIN)
    return x


def stored(kind, x):
    """The rows as a gallery of this kind stores them, up to the last bit of the normalisation: float32 unit rows, rounded to
    fp16 for "f16".  (The GPU tests read the stored rows back instead.)"""
    n = ivf_ref.normalise(x).astype(np.float32)
    return n.astype(np.float16).astype(np.float32) if kind == "f16" else n


def ivf_assign():
    """The list of every row of the IVF cases, scattered by a seeded permutation."""
    a = np.repeat(np.arange(len(IVF_LENGTHS)), IVF_LENGTHS)
    return a[np.random.default_rng(7).permutation(IVF_G)].astype(np.int64)


def ivf_groups(nq, Q=IVF_Q):
    """The groups of queries of one list that all Q queries probe: the pairs of a list ascend by query, nq at a time."""
    return [list(range(g0, min(Q, g0 + nq))) for g0 in range(0, Q, nq)]


# ---- the modelled bugs, on float64 operands: qn (Q, D) normalised queries, rows (G, D) as stored
def cut_after_first_trip(qn, rows, kind):
    """The row walk stops after its first trip."""
    f = FIRST_TRIP[kind]
    return qn[:, :f] @ rows[:, :f].T


def second_trip_rereads_first(qn, rows, kind):
    """Every later trip reads the row's elements of the first trip again (the trip offset never reaches the row pointer)."""
    f = FIRST_TRIP[kind]
    return qn @ rows[:, np.arange(rows.shape[1]) % f].T


def last_query_one_unit_early(qn, rows, kind, nq):
    """The last query of every group of two or more reads its LDS row one unit early: the last unit of its neighbour's padded
    row, then its own elements shifted by a unit."""
    Q, D = qn.shape
    L, u = ldq(D, kind), UNIT[kind]
    pad = np.zeros((Q, L))
    pad[:, :D] = qn
    S = qn @ rows.T
    for grp in ivf_groups(nq, Q):
        if len(grp) >= 2:
            last = grp[-1]
            seen = np.concatenate([pad[last - 1, L - u:], pad[last, : L - u]])[:D]
            S[last] = seen @ rows.T
    return S
