"""numpy float64 reference of the IVF search: the scores of every query against the rows of its probed lists only (every
other pair is -inf), the slab order of the candidates, and the top-k with the library's tie rule and pads."""
import numpy as np

NO_CAND = 1 << 62


def normalise(x, eps=1e-6):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), eps)


def lists_of(assign, nlist):
    """(offsets (nlist + 1,), order (G,)) of hand-made assignments: the rows of every list ascending."""
    assign = np.asarray(assign, np.int64)
    order = np.argsort(assign, kind="stable").astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]).astype(np.int64)
    return offsets, order


def probed_rows(offsets, order, probes_q):
    """The rows a query scans, in slab order: the members of its probed lists, list after list."""
    parts = [order[offsets[l]: offsets[l + 1]] for l in probes_q]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def eligible(G, Q, query_labels=None, gallery_labels=None, label_filter=None, exclude=None, idx_offset=0):
    ok = np.ones((Q, G), bool)
    if label_filter is not None:
        same = np.asarray(query_labels)[:, None] == np.asarray(gallery_labels)[None, :]
        ok &= same if label_filter == "same" else ~same
    if exclude is not None:
        ex = np.asarray(exclude, np.int64)
        for q in range(Q):
            if ex[q] >= 0 and 0 <= ex[q] - idx_offset < G:
                ok[q, ex[q] - idx_offset] = False
    return ok


def restricted_scores(rows, queries, offsets, order, probes, eps=1e-6, **filt):
    """S (Q, G) float64: normalise(queries) . rows (the rows as stored) where the row lies in a probed list of the query and
    is eligible, -inf elsewhere."""
    rows = np.asarray(rows, np.float64)
    full = normalise(queries, eps) @ rows.T
    Q, G = full.shape
    ok = eligible(G, Q, **filt)
    S = np.full((Q, G), -np.inf)
    for q in range(Q):
        r = probed_rows(offsets, order, probes[q])
        r = r[ok[q, r]]
        S[q, r] = full[q, r]
    return S


def topk(S, k, idx_offset=0):
    """(values (Q, k), indices (Q, k), gap (Q,)): descending, ties to the lower index, (-inf, -1) where fewer than k scores are
    finite; gap: the smallest difference between neighbours among the k + 1 best finite scores (inf with fewer than two)."""
    Q, G = S.shape
    idx = np.argsort(-S, axis=1, kind="stable")[:, :k]
    val = np.take_along_axis(S, idx, axis=1)
    pad = ~np.isfinite(val)
    idx = np.where(pad, -1, idx + idx_offset)
    if val.shape[1] < k:                            # k > G does not happen in the tests; keep the shapes honest
        raise ValueError("k exceeds the number of rows")
    gap = np.full(Q, np.inf)
    for q in range(Q):
        s = np.sort(S[q][np.isfinite(S[q])])[::-1][: k + 1]
        if s.size >= 2:
            gap[q] = float(np.min(s[:-1] - s[1:]))
    return val, idx.astype(np.int64), gap
