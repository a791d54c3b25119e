"""NumPy model of the fp4 gallery's numerical contract (include/mi355_retrieval.h), bit for bit: e2m1, the row quantiser, the
packing, the query's two e2m1 planes, the score of a (query, row) pair and the top-k order.  Every fp32 operation of the contract
is one float32 NumPy operation here; the dot products are float64 matrix products of the integers 2 * value(code) (exact:
|sum| < 2^53)."""
import numpy as np

from gallery_i8_ref import topk  # noqa: F401  (the order of mi355_rank_topk: the fp4 search selects as the int8 search does)

F32 = np.float32
MAGNITUDES = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=F32)       # by magnitude index; bit 3 of a code is the sign
TWICE = np.array([0, 1, 2, 3, 4, 6, 8, 12], dtype=np.int64)          # 2 * magnitude
TIES = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=F32)  # halfway between neighbours: each goes to the even index
SEGMENT = 128


def e2m1(a):
    """uint8 codes (0..15) of the float32 values a: the nearest magnitude, a tie to the even index, no negative zero."""
    a = np.asarray(a, dtype=F32)
    m = np.abs(a)
    idx = ((m > F32(0.25)).astype(np.uint8) + (m >= F32(0.75)) + (m > F32(1.25)) + (m >= F32(1.75)) + (m > F32(2.5))
           + (m >= F32(3.5)) + (m > F32(5))).astype(np.uint8)
    return (idx | np.where((a < 0) & (idx > 0), 8, 0)).astype(np.uint8)


def twice(codes):
    """int64: 2 * value(code), one of {0, +-1, 2, 3, 4, 6, 8, 12}."""
    codes = np.asarray(codes)
    return np.where(codes & 8, -TWICE[codes & 7], TWICE[codes & 7])


def value(codes):
    """float32 value of each code."""
    return (twice(codes).astype(F32) * F32(0.5)).astype(F32)


def stride(dim):
    return ((dim + 1) // 2 + SEGMENT - 1) // SEGMENT * SEGMENT


def pack(codes):
    """uint8 [R][ld]: dimension 2j in the low nibble of byte j, 2j + 1 in the high nibble, zeros from dim on."""
    R, D = codes.shape
    full = np.zeros((R, 2 * stride(D)), np.uint8)
    full[:, :D] = codes
    return (full[:, 0::2] | (full[:, 1::2] << 4)).astype(np.uint8)


def unpack(packed, dim):
    """uint8 codes [R][dim] of packed rows [R][>= ceil(dim / 2)]."""
    packed = np.asarray(packed, dtype=np.uint8)
    return np.stack((packed & 15, packed >> 4), axis=2).reshape(packed.shape[0], -1)[:, :dim]


def _amax(n):
    """(amax, bad, zero, live) per row of the float32 rows n."""
    amax = np.abs(n).max(axis=1) if n.shape[1] else np.zeros(n.shape[0], F32)
    bad = np.isnan(n).any(axis=1) | ~np.isfinite(amax)
    zero = ~bad & (amax < F32(1e-30))
    return amax, bad, zero, ~bad & ~zero


def quantize_rows(n):
    """(codes uint8 [R][D], one code per element, mult float32 [R]) of the float32 rows n (normalised already)."""
    n = np.ascontiguousarray(n, dtype=F32)
    with np.errstate(all="ignore"):
        amax, bad, zero, live = _amax(n)
        safe = np.where(live, amax, F32(1)).astype(F32)
        inv = (F32(6) / safe).astype(F32)
        codes = np.where(live[:, None], e2m1((n * inv[:, None]).astype(F32)), 0).astype(np.uint8)
        n2 = (twice(codes) ** 2).sum(axis=1)                          # an exact integer, <= 144 * D < 2^24
        root = np.sqrt((F32(0.25) * n2.astype(F32)).astype(F32)).astype(F32)
        mult = np.where(n2 > 0, F32(1) / np.where(n2 > 0, root, F32(1)), F32(0)).astype(F32)
    return codes, np.where(bad, F32(np.nan), np.where(zero, F32(0), mult)).astype(F32)


def residuals(qn, hi, s_q):
    """float32 r = fmaf(-value(hi), s_q, qn) / s_q of live queries (s_q finite and not 0)."""
    # the float64 difference is exact (value(hi) * s_q has 27 bits and lies within s_q of qn), so its float32 rounding is the fma
    d = (qn.astype(np.float64) - value(hi).astype(np.float64) * s_q.astype(np.float64)[:, None]).astype(F32)
    return (d / s_q[:, None]).astype(F32)


def query_planes(qn):
    """(hi uint8 [Q][D], lo uint8 [Q][D], s_q float32 [Q]) of the normalised float32 queries qn."""
    qn = np.ascontiguousarray(qn, dtype=F32)
    with np.errstate(all="ignore"):
        amax, bad, zero, live = _amax(qn)
        safe = np.where(live, amax, F32(1)).astype(F32)
        s = (safe / F32(6)).astype(F32)
        inv = (F32(6) / safe).astype(F32)
        q = np.where(live[:, None], qn, 0).astype(F32)
        hi = e2m1((q * inv[:, None]).astype(F32))
        lo = e2m1((F32(4) * residuals(q, hi, s)).astype(F32))
    hi, lo = np.where(live[:, None], hi, 0).astype(np.uint8), np.where(live[:, None], lo, 0).astype(np.uint8)
    return hi, lo, np.where(bad, F32(np.nan), np.where(zero, F32(0), s)).astype(F32)


def scores(hi, lo, s_q, codes, mult):
    """float32 [Q][G]: (fmaf(acc_lo, 0.25, acc_hi) * s_q) * mult."""
    c = twice(codes).astype(np.float64).T
    acc_hi = (twice(hi).astype(np.float64) @ c) / 4.0                 # multiples of 0.25 below 2^22: exact, and exact in float32
    acc_lo = (twice(lo).astype(np.float64) @ c) / 4.0
    assert (acc_hi.astype(F32) == acc_hi).all() and (acc_lo.astype(F32) == acc_lo).all()
    with np.errstate(all="ignore"):
        t = (acc_hi + acc_lo * 0.25).astype(F32)                      # exact sum, one rounding: the fma
        return ((t * s_q[:, None].astype(F32)).astype(F32) * mult[None, :].astype(F32)).astype(F32)


# ---- the planted mixture behind the recall bounds (test_gallery_fp4_ref.py on this model, test_gallery_fp4_gpu.py on the library)
MIX_D, MIX_G, MIX_CENTRES, MIX_Q, MIX_K, MIX_SHORTLIST = 256, 20000, 400, 200, 10, 30


def mixture(seed=0):
    """(rows float32 [G][D], queries float32 [Q][D]): unit-variance centres, rows and queries one unit of noise away from one."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((MIX_CENTRES, MIX_D))
    x = centres[rng.integers(0, MIX_CENTRES, MIX_G)] + rng.standard_normal((MIX_G, MIX_D))
    q = centres[rng.integers(0, MIX_CENTRES, MIX_Q)] + rng.standard_normal((MIX_Q, MIX_D))
    return x.astype(F32), q.astype(F32)


def mixture_recall(n, qn):
    """The model's search of the normalised queries qn over the normalised rows n against the float64 cosine: its shortlist
    (values, indices), raw recall@10 (the first 10 of the shortlist) and refined recall@10 (the shortlist rescored exactly)."""
    exact = np.argsort(-(qn.astype(np.float64) @ n.astype(np.float64).T), axis=1, kind="stable")[:, :MIX_K]
    codes, mult = quantize_rows(n)
    hi, lo, s_q = query_planes(qn)
    vals, idx = topk(scores(hi, lo, s_q, codes, mult), MIX_SHORTLIST)
    raw = np.mean([len(set(i[:MIX_K]) & set(e)) / MIX_K for i, e in zip(idx, exact)])
    refined = np.mean([len(set(i) & set(e)) / MIX_K for i, e in zip(idx, exact)])    # exact rescoring keeps what it is shown
    return dict(vals=vals, idx=idx, raw=float(raw), refined=float(refined))


def mixture_model():
    x, q = mixture()
    unit = lambda a: (a / np.sqrt((a.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(F32)  # noqa: E731
    return mixture_recall(unit(x), unit(q))
