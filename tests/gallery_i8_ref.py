"""NumPy model of the int8 gallery's numerical contract (include/mi355_retrieval.h), bit for bit: the row quantiser, the query's
two int8 planes, the score of a (query, row) pair and the top-k order.  Every fp32 operation of the contract is one float32
NumPy operation here; the integer dot products are float64 matrix products (exact: |sum| < 2^53)."""
import numpy as np

F32 = np.float32

# A row of amax = 127 * 2^e taken as it is has inv = 2^-e exactly, so n_i * inv is exact and these elements (times 2^e) are
# exact ties of rintf: (k + 0.5) for k = 0, 1, 2, 3, 125, 126 and their negatives; then the ends, and two elements off a tie
TIES = np.array([0.5, 1.5, 2.5, 3.5, 125.5, 126.5, -0.5, -1.5, -2.5, -3.5, -125.5, -126.5,
                 127.0, -127.0, 126.75, 0.25, -0.25], dtype=F32)
TIE_CODES = np.array([0, 2, 2, 4, 126, 126, 0, -2, -2, -4, -126, -126, 127, -127, 127, 0, 0], dtype=np.int8)   # half to even
TIE_EXPONENTS = (0, -3, 6)


def tie_rows(D):
    """(rows float32 [3][D], codes int8 [D], scales float32 [3]): TIES repeated along a row of D >= len(TIES) elements, scaled
    by 2^e for each e of TIE_EXPONENTS, with the codes and scales the contract gives them (the same codes for every e)."""
    assert D >= len(TIES)
    sel = np.arange(D) % len(TIES)
    rows = np.stack([TIES[sel] * F32(2.0 ** e) for e in TIE_EXPONENTS]).astype(F32)
    return rows, TIE_CODES[sel], np.array([2.0 ** e for e in TIE_EXPONENTS], dtype=F32)


def quantize_rows(n):
    """(codes int8 [R][D], scales float32 [R]) of the float32 rows n (normalised already)."""
    n = np.ascontiguousarray(n, dtype=F32)
    with np.errstate(all="ignore"):
        amax = np.abs(n).max(axis=1) if n.shape[1] else np.zeros(n.shape[0], F32)
        bad = np.isnan(n).any(axis=1) | ~np.isfinite(amax)
        zero = ~bad & (amax < F32(1e-30))
        live = ~bad & ~zero
        safe = np.where(live, amax, F32(1)).astype(F32)
        scale = (safe / F32(127)).astype(F32)
        inv = (F32(127) / safe).astype(F32)
        codes = np.clip(np.rint((n * inv[:, None]).astype(F32)), -127, 127)
    codes = np.where(live[:, None], codes, 0).astype(np.int8)
    scale = np.where(bad, F32(np.nan), np.where(zero, F32(0), scale)).astype(F32)
    return codes, scale


def query_planes(qn):
    """(hi int8 [Q][D], lo int8 [Q][D], s_q float32 [Q]) of the normalised float32 queries qn."""
    qn = np.ascontiguousarray(qn, dtype=F32)
    hi, s_q = quantize_rows(qn)
    live = np.isfinite(s_q) & (s_q != 0)
    with np.errstate(all="ignore"):
        safe = np.where(live, s_q, F32(1)).astype(F32)
        # fmaf(-hi, s_q, qn): the float64 difference is exact (hi * s_q has 31 bits and lies within s_q / 2 of qn)
        r = (np.where(live[:, None], qn, 0).astype(np.float64) - hi.astype(np.float64) * safe.astype(np.float64)[:, None]).astype(F32)
        mul = (F32(128) / safe).astype(F32)
        lo = np.clip(np.rint((r * mul[:, None]).astype(F32)), -127, 127)
    lo = np.where(live[:, None], lo, 0).astype(np.int8)
    return hi, lo, s_q


def scores(hi, lo, s_q, codes, s_g):
    """float32 [Q][G]: (fmaf(float(acc_lo), 2^-7, float(acc_hi)) * s_q) * s_g."""
    c = codes.astype(np.float64).T
    acc_hi = (hi.astype(np.float64) @ c).astype(F32)          # int32 -> float32, nearest even (float64 -> float32 is)
    acc_lo = (lo.astype(np.float64) @ c).astype(F32)
    with np.errstate(all="ignore"):
        t = (acc_hi.astype(np.float64) + acc_lo.astype(np.float64) / 128.0).astype(F32)   # exact sum, one rounding: the fma
        return ((t * s_q[:, None].astype(F32)).astype(F32) * s_g[None, :].astype(F32)).astype(F32)


def topk(s, k, mask=None):
    """(values float32 [Q][k], indices int64 [Q][k]): descending, NaN first, ties (and -0 / +0) to the lower index; with a
    boolean mask [Q][G] of eligible rows an ineligible row never appears and the slots past the eligible rows are (-inf, -1)."""
    s = np.asarray(s, dtype=F32)
    key = np.where(np.isnan(s), np.inf, s.astype(np.float64))
    elig = np.ones(s.shape, bool) if mask is None else np.asarray(mask, bool)
    key = np.where(elig, key, -np.inf)
    cols = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    order = np.lexsort((cols, ~elig, -key), axis=1)[:, :k]   # by score, then eligible rows first, then the lower index
    vals = np.take_along_axis(s, order, axis=1).astype(F32)
    idx = order.astype(np.int64)
    pad = np.arange(k)[None, :] >= elig.sum(axis=1)[:, None]
    return np.where(pad, F32(-np.inf), vals).astype(F32), np.where(pad, -1, idx)
