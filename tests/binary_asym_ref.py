"""NumPy model of the asymmetric binary search's numerical contract (include/mi355_retrieval.h, the block behind the binary
one), bit for bit: the gallery side is binary_ref's encoder unchanged, the query side is the int8 row quantiser applied to
r = n - center in float32, the distance is the Hamming distance weighted by the query's magnitudes - integers - and the score
is one float32 division.  No tolerance anywhere."""
import numpy as np

import binary_ref as R

F32 = R.F32


def query_codes(qn, center=None):
    """(u int8 [Q][dim], l1 int32 [Q], nan bool [Q]) of the normalised float32 queries qn: r = qn - center in float32,
    amax = max |r|, inv = float32(127) / amax, u = clamp(rint(r * inv), -127, 127).  A NaN in r or a non-finite amax: a NaN
    query, codes 0.  amax < 1e-30: codes 0."""
    qn = np.ascontiguousarray(qn, dtype=F32)
    Q, dim = qn.shape
    c = np.zeros(dim, F32) if center is None else np.ascontiguousarray(center, dtype=F32)
    u = np.zeros((Q, dim), np.int8)
    nan = np.zeros(Q, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (qn - c[None, :]).astype(F32)
        for i in range(Q):
            amax = F32(np.abs(r[i]).max()) if not np.isnan(r[i]).any() else F32(np.nan)
            if np.isnan(amax) or not amax <= np.finfo(F32).max:
                nan[i] = True
                continue
            if amax < F32(1e-30):
                continue
            inv = F32(127.0) / amax
            u[i] = np.clip(np.rint((r[i] * inv).astype(F32)), -127.0, 127.0).astype(np.int8)
    return u, np.abs(u.astype(np.int64)).sum(axis=1).astype(np.int32), nan


def bits(gcodes, dim):
    """uint8 [G][dim]: bit j of every code row."""
    g = np.ascontiguousarray(gcodes, dtype=np.uint32)
    b = (g[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return b.reshape(g.shape[0], -1)[:, :dim].astype(np.uint8)


def weighted_distances(u, gcodes, qnan=None):
    """int32 [Q][G]: m = sum_j |u_j| * [(u_j > 0 and bit_j == 0) or (u_j < 0 and bit_j == 1)], computed as Upos - P with P the
    sum of u over the set bits; -1 in the rows of the queries flagged in qnan."""
    u = np.asarray(u, np.int64)
    b = bits(gcodes, u.shape[1]).astype(np.int64)
    upos = np.maximum(u, 0).sum(axis=1)
    m = (upos[:, None] - u @ b.T).astype(np.int32)
    if qnan is not None:
        m[np.asarray(qnan, bool)] = -1
    return m


def weighted_distances_by_definition(u, gcodes):
    """The same integers straight from the definition (a check of the model on small shapes)."""
    u = np.asarray(u, np.int64)
    b = bits(gcodes, u.shape[1]).astype(bool)
    miss = ((u[:, None, :] > 0) & ~b[None, :, :]) | ((u[:, None, :] < 0) & b[None, :, :])
    return (np.abs(u)[:, None, :] * miss).sum(axis=2).astype(np.int32)


def scores(m, l1):
    """float32 [Q][G]: float32(L1 - 2 m) / float32(L1), one division; 0 where L1 == 0; NaN where m is -1 (a NaN query)."""
    m = np.asarray(m, np.int64)
    l1 = np.asarray(l1, np.int64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (l1 - 2 * m).astype(F32) / np.broadcast_to(l1, m.shape).astype(F32)
    s = np.where(l1 == 0, F32(0.0), s)
    return np.where(m < 0, F32(np.nan), s).astype(F32)


def model(qn, gcodes, center=None):
    """(m, s, u, l1, nan) of the normalised queries against the code rows."""
    u, l1, nan = query_codes(qn, center)
    m = weighted_distances(u, gcodes, nan)
    return m, scores(m, l1), u, l1, nan


def refined_recall(n, qn, key, k=10, shortlist=100):
    """binary_ref.refined_recall with the shortlist taken by `key` (float32 [Q][G] scores, higher first, ties to the lower
    row): recall@k against the float64 cosine top-k of the unit rows, the shortlist rescored exactly and cut to k."""
    cos = qn.astype(np.float64) @ n.astype(np.float64).T
    want = np.argsort(-cos, axis=1, kind="stable")[:, :k]
    _, short = R.select(key, shortlist)
    re = np.take_along_axis(cos, short, axis=1)
    got = np.take_along_axis(short, np.argsort(-re, axis=1, kind="stable")[:, :k], axis=1)
    return float(np.mean([len(set(a) & set(b)) / float(k) for a, b in zip(got.tolist(), want.tolist())]))


def mixture_rows(seed, pooled):
    """(n, qn) float32 unit rows of the planted mixture, raw or pooled."""
    x, q = R.planted_mixture(seed)
    if pooled:
        x, q = R.pooled(x), R.pooled(q)
    return R.normalize(x), R.normalize(q)
