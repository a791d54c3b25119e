"""Test helper: float64 numpy reference of alpha query expansion (alpha-QE) and database-side augmentation (DBA), Radenovic,
Tolias and Chum, TPAMI 2018, with the library's slot rule (include/mi355_retrieval.h, mi355_expand_rows):

    x   = base + sum_j w_j * row(i_j),   w_j = v_j ** alpha for a slot with v_j > 0 and a real row (others skipped)
    out = x / max(|x|, eps)

plus the float64 cosine top-k the ranking tests compare against, and the four retrieval metrics (Musgrave et al. 2020)."""
from __future__ import annotations

import numpy as np

EPS = 1e-6


KERNEL_ROWS, KERNEL_GALLERY = 37, 300


def kernel_case(D, n, seed):
    """Inputs of the kernel tests: queries (37, D) with norms about 0.4 .. 0.7 or 1.5 .. 3, gallery (300, D) whose LAST row is NaN, and (37, n)
    neighbour lists holding (-inf, -1) pads, negative and NaN scores (the NaN row sits only behind those), a row outside the
    gallery, and positive scores in [0.3, 1] on real rows.  Returns numpy (q, g, vals, idx, rows_with_pads)."""
    rng = np.random.default_rng(seed)
    Rr, G = KERNEL_ROWS, KERNEL_GALLERY
    scale = np.where(rng.random((Rr, 1)) < 0.5, rng.uniform(0.4, 0.7, (Rr, 1)), rng.uniform(1.5, 3.0, (Rr, 1)))
    q = (rng.standard_normal((Rr, D)) * scale / np.sqrt(D)).astype(np.float32)
    g = rng.standard_normal((G, D)).astype(np.float32)
    if D == 1:                                               # one dimension: same signs, so x = qn + sum w r never cancels
        q, g = np.abs(q), np.abs(g)
    g[G - 1] = np.nan
    vals = rng.uniform(0.3, 1.0, (Rr, n)).astype(np.float32)
    idx = rng.integers(0, G - 1, (Rr, n)).astype(np.int64)
    vals = -np.sort(-vals, axis=1)                           # rank order (the kernel does not depend on it)
    pads = np.zeros(Rr, bool)
    for r in range(Rr):
        kind = r % 6
        if n == 1 and kind in (1, 2, 3):
            kind = 0 if r % 2 else kind
        if kind == 1:                                        # filtered search: tail of pads
            t = max(n // 2, n - 3)
            vals[r, t:], idx[r, t:] = -np.inf, -1
            pads[r] = True
        elif kind == 2:                                      # a negative score, the NaN row behind it
            vals[r, -1], idx[r, -1] = -0.3, G - 1
        elif kind == 3:                                      # a NaN score, the NaN row behind it
            vals[r, -1], idx[r, -1] = np.nan, G - 1
        elif kind == 4:                                      # a row outside the gallery with a positive score
            idx[r, 0] = G + 5
        elif kind == 5 and n == 1:                           # the only slot is a pad: the output is qn
            vals[r, 0], idx[r, 0] = -np.inf, -1
            pads[r] = True
    return q, g, vals, idx, pads


def normalize(x, eps=EPS):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), eps)


def slot_weights(vals, idx, alpha, rows, idx_offset=0):
    """(w, local, used): float64 weights, local rows and the mask of used slots of (R, n) neighbour lists."""
    vals = np.asarray(vals, dtype=np.float64)
    local = np.asarray(idx, dtype=np.int64) - idx_offset
    with np.errstate(invalid="ignore"):
        used = (vals > 0) & (local >= 0) & (local < rows)
    w = np.where(used, np.power(np.where(used, vals, 1.0), float(alpha)), 0.0)
    return w, np.where(used, local, 0), used


def expand_sum(base, gallery_rows, vals, idx, alpha, normalize_base=True, idx_offset=0, eps=EPS):
    """The un-normalised sum x (R, D) in float64.  A skipped slot's row is never touched (a NaN row behind it stays out)."""
    g = np.asarray(gallery_rows, dtype=np.float64)
    x = normalize(base, eps) if normalize_base else np.array(base, dtype=np.float64)
    w, local, used = slot_weights(vals, idx, alpha, g.shape[0], idx_offset)
    for r in range(x.shape[0]):
        for j in np.nonzero(used[r])[0]:
            x[r] += w[r, j] * g[local[r, j]]
    return x


def expand(base, gallery_rows, vals, idx, alpha, normalize_base=True, idx_offset=0, eps=EPS):
    return normalize(expand_sum(base, gallery_rows, vals, idx, alpha, normalize_base, idx_offset, eps), eps)


def cosine_topk(q, g, k, exclude=None):
    """float64 top-k of normalised q against normalised g: (vals, idx, all scores); ties to the lower index; ``exclude`` (Q,)
    leaves out one row per query, slots beyond the eligible rows are (-inf, -1)."""
    S = normalize(q) @ normalize(g).T
    if exclude is not None:
        S = S.copy()
        S[np.arange(S.shape[0]), exclude] = -np.inf
    order = np.lexsort((np.broadcast_to(np.arange(S.shape[1]), S.shape), -S), axis=1)[:, :k]
    v = np.take_along_axis(S, order, 1)
    i = np.where(np.isfinite(v), order, -1)
    return v, i, S


def gaps(S, k, exclude=None):
    """Per query: the smallest gap between consecutive scores among the first k + 1 ranks (certification of a top-k)."""
    S = S.copy()
    if exclude is not None:
        S[np.arange(S.shape[0]), exclude] = -np.inf
    top = -np.sort(-S, axis=1)[:, : k + 1]
    return np.diff(-top, axis=1).min(1)


def qe_pipeline(q, g, n, alpha, k, exclude=None):
    """float64 alpha-QE search: round 1 top-n, expansion over the normalised gallery, round 2 top-k.  Returns
    (round-1 (v, i, S), expanded queries, round-2 (v, i, S))."""
    r1 = cosine_topk(q, g, n, exclude)
    qe = expand(q, normalize(g), r1[0], r1[1], alpha)
    return r1, qe, cosine_topk(qe, g, k, exclude)


def retrieval_metrics(idx, ql, gl, R, ks):
    """precision@1, recall@K, R-precision and MAP@R of ranked rows idx (Q, k), float64, queries with R = 0 left out."""
    idx, ql, gl, R = (np.asarray(t) for t in (idx, ql, gl, R))
    G = gl.shape[0]
    valid = R > 0
    rel = np.where((idx >= 0) & (idx < G), gl[np.clip(idx, 0, G - 1)] == ql[:, None], False)
    rp = np.zeros(len(R))
    mapr = np.zeros(len(R))
    for q in np.nonzero(valid)[0]:
        r = int(R[q])
        rr = rel[q, :r].astype(np.float64)
        rp[q] = rr.sum() / r
        mapr[q] = (rr * np.cumsum(rr) / np.arange(1, r + 1)).sum() / r
    m = lambda x: x[valid].mean()  # noqa: E731
    return {"precision_at_1": m(rel[:, 0].astype(np.float64)),
            "recall_at_k": {K: m(rel[:, :K].any(1).astype(np.float64)) for K in ks},
            "r_precision": m(rp), "map_at_r": m(mapr)}
