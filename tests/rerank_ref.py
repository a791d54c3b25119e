"""Test helper: float64 numpy reference of k-reciprocal re-ranking (Zhong, Zheng, Cao and Li, CVPR 2017) in the library's
gallery-graph variant (include/mi355_retrieval.h, mi355_kr_*), written with Python sets, dicts and dense loops.

    nn(g), nv(g)  top-k1 OTHER gallery rows of gallery row g and their scores; tau(g) = nv(g)[k1 - 1]; h = (k1 + 1) // 2
    R(g)   = {g} | {j in nn(g) : g in nn(j)}                 R(q) = {j in nn(q) : nv(q)[j] >= tau(j)}  (fp32 comparison)
    R_h(c) = {c} | {j in nn_h(c) : c in nn_h(j)}
    R*(r)  = R(r) | U {R_h(c) : c in R(r), 3 |R_h(c) & R(r)| > 2 |R_h(c)|}
    V(r)[j]  = exp(-(1 - s(r, j))) / sum over R*(r)
    V'(g)    = mean of V over the first k2 of [g, nn(g) ...];   V'(q) = (V(q) + sum of V over the first k2 - 1 of nn(q)) / k2
    s*(q, g) = 1 - ((1 - lam) dJ + lam (1 - s(q, g))),  dJ = 1 - m / (2 - m),  m = sum_c min(V'(q)[c], V'(g)[c])

Sparse rows are dicts {column: value}; ``to_csr`` flattens a list of them (ascending columns) for comparison with the kernels.

Lists given by hand may hold what a search never returns.  The reference skips it where the kernels do (csrc/rerank.hip):

    an id outside [0, G) in a list or in the graph is no member, no candidate and no reciprocal neighbour;
    a gallery row that lists itself gains nothing from it (it is in its own R already), and in R_h(c) the entry c counts once;
    a repeated id in a list counts once: its FIRST occurrence decides (for a query row, that occurrence's score against tau);
    ``weights``: a column outside [0, G) gets the weight 0 and stays out of the row's sum;
    ``local_qe``: a source outside [0, G) is absent - the sum is still divided by k2 - and a repeated source is added once per
    occurrence;
    ``scores``: a slot outside [0, G), not only a negative one, is -inf."""
from __future__ import annotations

import numpy as np


def _valid(j, G):
    return 0 <= int(j) < G


def recip_h(graph, c, h):
    """R_h(c) as a set."""
    G = len(graph)
    return {int(c)} | {int(j) for j in graph[c][:h] if _valid(j, G) and c in graph[int(j)][:h]}


def base_set(r, nn_row, graph, nv_row=None, tau=None):
    """R(r): gallery row r (nv_row None) or a query with its scores nv_row (compared as given: pass float32 arrays)."""
    G = len(graph)
    if nv_row is None:
        return {int(r)} | {int(j) for j in nn_row if _valid(j, G) and r in graph[int(j)]}
    out, seen = set(), set()
    for t, j in enumerate(nn_row):
        j = int(j)
        if not _valid(j, G) or j in seen:
            continue
        seen.add(j)
        if nv_row[t] >= tau[j]:
            out.add(j)
    return out


def expanded_set(base, graph, h):
    out = set(base)
    for c in sorted(base):
        rh = recip_h(graph, c, h)
        if 3 * len(rh & base) > 2 * len(rh):
            out |= rh
    return out


def sets(lists, graph, list_vals=None, tau=None):
    """R*(r) of every row of ``lists`` (R, k1) as sorted lists; gallery rows when list_vals is None (lists is then the graph)."""
    graph = np.asarray(graph)
    k1 = graph.shape[1]
    h = (k1 + 1) // 2
    out = []
    for r in range(len(lists)):
        base = base_set(r, lists[r], graph, None if list_vals is None else list_vals[r], tau)
        out.append(sorted(expanded_set(base, graph, h)))
    return out


def to_csr(rows, with_vals=False):
    """Rows as sorted column lists (or dicts) -> (offsets int64, cols int32[, vals float64])."""
    offsets = np.zeros(len(rows) + 1, np.int64)
    cols, vals = [], []
    for r, row in enumerate(rows):
        keys = sorted(row)
        offsets[r + 1] = offsets[r] + len(keys)
        cols += keys
        if with_vals:
            vals += [row[c] for c in keys]
    cols = np.asarray(cols, np.int32).reshape(-1)
    return (offsets, cols, np.asarray(vals, np.float64)) if with_vals else (offsets, cols)


def from_csr(offsets, cols, vals):
    return [{int(c): float(v) for c, v in zip(cols[offsets[r]:offsets[r + 1]], vals[offsets[r]:offsets[r + 1]])}
            for r in range(len(offsets) - 1)]


def weights(rows, gallery, col_sets):
    """V as a list of dicts: rows (R, D) and gallery (G, D) float64 NORMALISED rows, col_sets the R*(r).  A gallery row that is in
    no set is never touched."""
    rows, gallery = np.asarray(rows, np.float64), np.asarray(gallery, np.float64)
    G = len(gallery)
    out = []
    for r, cs in enumerate(col_sets):
        e = {int(j): np.exp(-(1.0 - float(rows[r] @ gallery[int(j)]))) for j in cs if _valid(j, G)}
        tot = sum(e[j] for j in sorted(e))
        out.append({int(j): e[int(j)] / tot if int(j) in e else 0.0 for j in cs})
    return out


def local_qe(own, gallery_V, lists, k2):
    """V'(r) = (own[r] + sum of gallery_V over lists[r][: k2 - 1]) / k2 as dicts."""
    out = []
    for r, v in enumerate(own):
        acc = dict(v)
        for j in lists[r][: k2 - 1]:
            if not _valid(j, len(gallery_V)):
                continue
            for c, x in gallery_V[int(j)].items():
                acc[c] = acc.get(c, 0.0) + x
        out.append({c: x / k2 for c, x in acc.items()})
    return out


def scores(vq2, vg2, short_vals, short_idx, lam):
    """s* (Q, K) float64; pads (an index outside [0, G)) are -inf."""
    short_vals = np.asarray(short_vals, np.float64)
    out = np.full(short_vals.shape, -np.inf)
    for q in range(out.shape[0]):
        a = vq2[q]
        for p in range(out.shape[1]):
            g = int(short_idx[q, p])
            if not _valid(g, len(vg2)):
                continue
            b = vg2[g]
            m = sum(min(a[c], b[c]) for c in sorted(a.keys() & b.keys()))
            dj = 1.0 - m / (2.0 - m)
            out[q, p] = 1.0 - ((1.0 - lam) * dj + lam * (1.0 - short_vals[q, p]))
    return out


def rank_shortlist(sstar, short_idx, k):
    """Top-k of the shortlist by descending s*, ties to the earlier position: (values, indices, positions)."""
    pos = np.argsort(-sstar, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(sstar, pos, 1), np.take_along_axis(np.asarray(short_idx), pos, 1), pos


def gaps(sstar, k):
    """Per query: the smallest gap between adjacent s* among ranks 1 .. k + 1 (certification of the top-k; inf with one rank)."""
    top = -np.sort(-sstar, axis=1)[:, : k + 1]
    top = np.where(np.isfinite(top), top, -1e9)
    return np.diff(-top, axis=1).min(1) if top.shape[1] > 1 else np.full(top.shape[0], np.inf)


def gallery_index(gn, nn, k2):
    """(V, V') of every gallery row from its normalised float64 rows ``gn`` and graph ``nn`` (G, k1)."""
    V = weights(gn, gn, sets(nn, nn))
    return V, local_qe(V, V, nn, k2)


def pipeline(qn, gn, graph_nv, graph_nn, q_nv, q_nn, short_vals, short_idx, k2, lam):
    """The whole re-ranking in float64 from given lists (the GPU's own round-1 lists, or ``knn`` below): s* (Q, K)."""
    tau = np.asarray(graph_nv)[:, -1]
    V, V2 = gallery_index(gn, graph_nn, k2)
    Vq = weights(qn, gn, sets(q_nn, graph_nn, q_nv, tau))
    Vq2 = local_qe(Vq, V, q_nn, k2)
    return scores(Vq2, V2, short_vals, short_idx, lam)


def knn(qn, gn, k, exclude=None):
    """float64 cosine top-k of normalised rows (ties to the lower index); scores returned as float32, as the library's lists."""
    S = np.asarray(qn, np.float64) @ np.asarray(gn, np.float64).T
    if exclude is not None:
        S[np.arange(S.shape[0]), exclude] = -np.inf
    order = np.lexsort((np.broadcast_to(np.arange(S.shape[1]), S.shape), -S), axis=1)[:, :k]
    return np.take_along_axis(S, order, 1).astype(np.float32), order.astype(np.int64)
