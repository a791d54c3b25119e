"""The inputs of the quantised galleries' extreme cases (test_quantised_extremes_gpu.py on the GPU, the premises alone in
test_quantised_extremes_args.py without one): saturated int8 rows whose integer sums reach their ceiling, galleries one partial
trip longer than the grid of the int8 and the fp4 GEMV, and a zero and a NaN query.  NumPy only.

The constants below are restated from the code they aim at: rank_topk_rows (rows_gemm.h) launches min(cdiv(G, 4), 4096)
workgroups of four waves for a GEMV, k_cos_gemv_i8 gives a wave one row per trip and k_cos_gemv_fp4 GEMV_ROWS = 4."""
import numpy as np

F32 = np.float32

# ---- 1. saturated int8 rows
SAT_DIMS = (4096, 65536)
SAT_G, SAT_Q = 130, 8
SAT_CASES = ((1, 130), (4, 3), (4, 130), (5, 3), (8, 130))          # (Q, k)
I8_GEMV_LDS, I8_SEGMENT = 64 * 1024, 128


def saturated(D, rows, seed):
    """rows float32 rows of +-1 with a trailing run of +-1/254 from column D - 1 - 3 r on (codes +-127, then a tie at 0.5); the
    first half of the rows all positive (the sums reach 127^2 D), the rest with seeded random signs.  Odd rows hold 126.5/127
    where even rows hold 1, but for their first element: as queries their hi plane is a tie (126 or 127) and their lo plane
    +-64 or +-63."""
    x = np.ones((rows, D), F32)
    x[1::2] = F32(126.5) / F32(127)
    x[:, 0] = 1.0
    for r in range(rows):
        x[r, D - 1 - 3 * r:] = F32(1) / F32(254)
    sign = np.where(np.random.default_rng(seed).random((rows - rows // 2, D)) < 0.5, -1.0, 1.0).astype(F32)
    x[rows // 2:] *= sign
    return x


def i8_gemv_runs(Q, D):
    """Whether Q queries of dim D take the int8 GEMV (i8_gemv): Q <= 4 and their two planes fit the GEMV's LDS."""
    ld = (D + I8_SEGMENT - 1) // I8_SEGMENT * I8_SEGMENT
    return Q <= 4 and Q * 2 * ld <= I8_GEMV_LDS


def saturated_sums(hi, lo, codes):
    """(max |acc_hi| / (127^2 D), max |acc_lo| / (64 * 127 D), acc_hi, acc_lo) with the sums in int64."""
    D = codes.shape[1]
    c = codes.astype(np.int64).T
    acc_hi, acc_lo = hi.astype(np.int64) @ c, lo.astype(np.int64) @ c
    return float(np.abs(acc_hi).max()) / (127 * 127 * D), float(np.abs(acc_lo).max()) / (64 * 127 * D), acc_hi, acc_lo


def assert_saturated(hi, lo, codes):
    """What the saturated case is there for, on the model's planes and codes; returns the two ratios."""
    r_hi, r_lo, acc_hi, acc_lo = saturated_sums(hi, lo, codes)
    assert r_hi >= 0.99 and r_lo >= 0.99, (r_hi, r_lo)
    assert np.abs(acc_hi).max() < 2 ** 31 and np.abs(acc_lo).max() < 2 ** 31
    return r_hi, r_lo


# ---- 3. the GEMV's second trip through its grid
GEMV_MAX_BLOCKS, GEMV_BLOCK_WAVES, FP4_GEMV_ROWS = 4096, 4, 4
GEMV_WAVES = GEMV_MAX_BLOCKS * GEMV_BLOCK_WAVES                      # 16384
WRAP_ROWS_PER_TRIP = {"i8": GEMV_WAVES, "fp4": GEMV_WAVES * FP4_GEMV_ROWS}
WRAP_EXTRA, WRAP_D, WRAP_Q, WRAP_KS = 5, 70, 4, (3, 150)
WRAP_G = {kind: n + WRAP_EXTRA for kind, n in WRAP_ROWS_PER_TRIP.items()}


def gemv_blocks(G):
    return min(-(-G // 4), GEMV_MAX_BLOCKS)


def second_trip(kind, G):
    """{wave: rows of its second trip} of the kind's GEMV over G rows."""
    per = 1 if kind == "i8" else FP4_GEMV_ROWS
    nwaves = gemv_blocks(G) * GEMV_BLOCK_WAVES
    out = {}
    for w in range(nwaves):
        g0 = (w + nwaves) * per
        if g0 < G:
            out[w] = list(range(g0, min(G, g0 + per)))
    return out


def wrap_case(kind):
    """(rows [G][70], queries [4][70]) float32: seeded Gaussian rows, the last five around one shared direction (cosine about
    0.8 among them, far above any other row's), query j = row G - 5 + j plus a little noise: every query's best row, and more
    of its best rows, are rows of the second trip."""
    G = WRAP_G[kind]
    rng = np.random.default_rng(G)
    x = rng.standard_normal((G, WRAP_D))
    x[G - WRAP_EXTRA:] += 2.0 * rng.standard_normal(WRAP_D)[None, :]
    q = x[G - WRAP_EXTRA: G - WRAP_EXTRA + WRAP_Q] + 0.05 * rng.standard_normal((WRAP_Q, WRAP_D))
    return x.astype(F32), q.astype(F32)


def assert_wrapped(kind, top_idx):
    """On the model's top-150 indices [Q][150]: every query's best row is a row of the second trip, and so are at least two
    of its 150 (here: all five, so the row a wave takes alone is compared too)."""
    G = WRAP_G[kind]
    late = top_idx >= G - WRAP_EXTRA
    assert late[:, 0].all() and (late.sum(axis=1) >= 2).all()
    assert (top_idx[:, 0] == G - WRAP_EXTRA + np.arange(top_idx.shape[0])).all() and (late.sum(axis=1) == WRAP_EXTRA).all()


# ---- 4. a zero and a NaN query
SPECIAL_G, SPECIAL_D, SPECIAL_NAN_ROW, ZERO_Q, NAN_Q = 300, 200, 7, 1, 2
SPECIAL_QS, SPECIAL_KS = (3, 6), (4, 150)                            # the GEMV and the GEMM


def special_case():
    """(rows [300][200] with a NaN in row 7, queries [6][200]: query 1 all zeros, query 2 with a NaN element) float32."""
    rng = np.random.default_rng(41)
    x, q = rng.standard_normal((SPECIAL_G, SPECIAL_D)).astype(F32), rng.standard_normal((max(SPECIAL_QS), SPECIAL_D)).astype(F32)
    x[SPECIAL_NAN_ROW, 3] = np.nan
    q[ZERO_Q] = 0.0
    q[NAN_Q, 5] = np.nan
    return x, q


def normalise(x, eps=1e-6):
    """float32 unit rows by a float64 norm: the library's own rows up to a rounding (the GPU tests read the library's)."""
    x = x.astype(F32)
    with np.errstate(all="ignore"):
        return (x / np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)), eps)[:, None].astype(F32)).astype(F32)
