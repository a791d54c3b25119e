"""Spherical k-means on resident rows and the clustering scores metric-learning papers report next to Recall@K
(NMI, purity, pairwise F1 with K = the number of classes; Musgrave et al. 2020, "A Metric Learning Reality Check").

* ``assign_clusters`` ..... nearest centroid of every row: one more epilogue of the tiled cosine GEMM (``mi355_nearest_centroid``)
* ``update_centroids`` .... members of every cluster as CSR, then ``normalise(sum of the member rows)`` in float64
                            (``mi355_centroid_update``), the same bits on every run
* ``spherical_kmeans`` .... the loop of the two, from seeded distinct rows or a given start
* ``contingency`` ......... the table of two labelings (``mi355_contingency``)
* ``clustering_metrics`` .. NMI, purity, pairwise precision / recall / F1 of that table (host float64)
* ``dbscan`` .............. DBSCAN on cosine similarity without a pair list: two sweeps of the cosine GEMM (a degree epilogue, a
                            link epilogue over a lock-free union-find: ``mi355_dbscan_*``), the same bits on every run
* ``connected_components``  ``dbscan`` with ``min_samples=1``: the components of the threshold graph

The rows are a (N, D) device tensor or a ``Gallery`` (fp32 or fp16), whose resident rows are read where they lie.  Out of
scope here: k-means++ seeding, mini-batches, ``ShardedGallery``.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import rank as _rank
from . import synth
from ._lib import MI355Error, check, lib, require_cuda, stream_ptr

_EPS = _rank._EPS
_ASSIGN = {torch.float32: ("mi355_nearest_centroid", "mi355_nearest_centroid_workspace_bytes"),
           torch.float16: ("mi355_nearest_centroid_f16", "mi355_nearest_centroid_f16_workspace_bytes")}
_UPDATE = {torch.float32: ("mi355_centroid_update", "mi355_centroid_update_workspace_bytes"),
           torch.float16: ("mi355_centroid_update_f16", "mi355_centroid_update_f16_workspace_bytes")}


class KMeansResult(NamedTuple):
    centroids: torch.Tensor       # (K, D) fp32: unit rows, except a row no update replaced (``iters=0``, an empty or kept
                                  # cluster), which is the start's row as given (a seeded start of a raw tensor: a raw row)
    assignments: torch.Tensor     # (N,) int64, the nearest of ``centroids``
    scores: torch.Tensor          # (N,) fp32, the cosine to it
    counts: torch.Tensor          # (K,) int64 rows per cluster
    members: tuple                # (offsets (K+1,), order (N,)) int64: rows of cluster k = order[offsets[k]:offsets[k+1]], ascending
    objective: float              # mean cosine of a row to its own centroid
    iterations: int               # assignment passes run
    converged: bool               # the last pass changed no assignment


def _rows_of(rows, name: str = "rows") -> "_rank._Rows":
    """The rows a clustering call reads: the resident rows of a ``Gallery`` where they lie, or a (N, D) fp32 device tensor
    (not normalised; made contiguous if it is not)."""
    if isinstance(rows, _rank.Gallery):
        rows = rows._resident()
    if isinstance(rows, _rank._Rows):
        if rows.buf is None:
            raise MI355Error(f"{name}: a prepared gallery without its rows cannot be clustered")
        return rows
    if not torch.is_tensor(rows):
        raise MI355Error(f"{name} must be a tensor or a Gallery, got {type(rows).__name__}")
    return _rank._Rows.of(rows)


def _centroids_of(centroids, src, name: str = "centroids") -> torch.Tensor:
    if not torch.is_tensor(centroids):
        raise MI355Error(f"{name} must be a tensor, got {type(centroids).__name__}")
    c = _rank._f32c(centroids, name)
    if c.dim() != 2 or c.shape[0] < 1:
        raise MI355Error(f"{name} must be (K, D) with K >= 1, got {tuple(c.shape)}")
    _rank._check_qg(c, src)
    return c


def _check_rows(src) -> None:
    if src.rows < 1 or src.dim < 1:
        raise MI355Error(f"clustering needs at least one row and one column, got {src.shape}")


def _check_k(n_clusters, N: int) -> int:
    if not _rank._is_int(n_clusters):
        raise MI355Error(f"n_clusters must be an integer, got {n_clusters!r}")
    if not 1 <= n_clusters <= N:
        raise MI355Error(f"n_clusters={n_clusters} outside [1, {N}] (the number of rows)")
    return int(n_clusters)


def _assign(src, c: torch.Tensor, block, eps: float):
    N, dev = src.rows, src.device
    if block is not None and (not _rank._is_int(block) or block < 1):
        raise MI355Error(f"block must be a positive integer, got {block!r}")
    assign = torch.empty(N, dtype=torch.int64, device=dev)
    score = torch.empty(N, dtype=torch.float32, device=dev)
    L = lib()
    entry, ws_bytes = _ASSIGN[src.dtype]
    ws = _rank._ws.get(dev, getattr(L, ws_bytes)(c.shape[0], N, src.dim))
    with torch.cuda.device(dev):
        check(getattr(L, entry)(c.data_ptr(), c.shape[0], *src.c_args(), eps, 0 if block is None else int(block),
                                assign.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(dev)))
    return assign, score


def assign_clusters(rows, centroids: torch.Tensor, *, block: int | None = None, eps: float = _EPS):
    """(assign (N,) int64, score (N,) fp32): for every row the centroid with the highest cosine and that cosine; equal
    scores go to the lower centroid.  ``rows``: a ``Gallery`` (its resident rows, fp32 or fp16, read in place) or a (N, D) fp32
    device tensor (its norms taken on the fly, not normalised into a copy; a contiguous tensor is read where it lies, a
    strided one is first copied contiguous).  ``centroids`` (K, D) need not be normalised.  Every score has
    the bits of the gallery's own search of the centroids.  ``block``: centroids per GEMM call (default: all that fit);
    the result does not depend on it."""
    src = _rows_of(rows)
    c = _centroids_of(centroids, src)
    _check_rows(src)
    return _assign(src, c, block, eps)


def _update(src, assign: torch.Tensor, K: int, previous: torch.Tensor, eps: float):
    """``update_centroids`` on normalised rows ``src`` (fp32 or fp16 ``_Rows``)."""
    N, D, dev = src.rows, src.dim, src.device
    out = torch.empty((K, D), dtype=torch.float32, device=dev)
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
    order = torch.empty(N, dtype=torch.int64, device=dev)
    L = lib()
    entry, ws_bytes = _UPDATE[src.dtype]
    ws = _rank._ws.get(dev, getattr(L, ws_bytes)(N, K, D))
    with torch.cuda.device(dev):
        check(getattr(L, entry)(src.buf.data_ptr(), N, D, assign.data_ptr(), K, previous.data_ptr(), eps, out.data_ptr(),
                                counts.data_ptr(), offsets.data_ptr(), order.data_ptr(), ws.data_ptr(), ws.numel(),
                                stream_ptr(dev)))
    return out, counts, (offsets, order)


def _unit_rows(src, eps: float):
    """``src`` as normalised rows: a Gallery's are already; a raw tensor is normalised into a temporary (N x D fp32)."""
    if src.normalized or src.dtype == torch.float16:
        return src
    return _rank._Rows(_rank.l2_normalize_rows(src.buf, eps), src.rows, src.dim, True)


def _update_args(src, assign, n_clusters, previous):
    _check_rows(src)
    K = _check_k(n_clusters, src.rows)
    a = _rank._int64_on(assign, "assign", src.rows, src.device)
    p = _centroids_of(previous, src, "previous")
    if p.shape[0] != K:
        raise MI355Error(f"previous must be ({K}, {src.dim}), got {tuple(p.shape)}")
    return K, a, p


def update_centroids(rows, assign: torch.Tensor, n_clusters: int, previous: torch.Tensor, *, eps: float = _EPS):
    """(centroids (K, D) fp32, counts (K,) int64, members): centroid k = ``normalise(sum of the normalised rows assigned to
    k)``, summed in float64 in ascending row order and rounded once to fp32.  A cluster without rows (or whose sum is shorter
    than ``eps``) keeps ``previous[k]`` bit for bit.  ``members = (offsets, order)`` lists every cluster's rows (CSR,
    ascending).  A ``Gallery``'s rows are used in place (fp16 widened exactly); a raw tensor is first normalised with
    ``l2_normalize_rows`` into a temporary copy (N x D fp32).  ``assign`` values outside [0, n_clusters) raise.  The same
    bits on every run."""
    src = _rows_of(rows)
    K, a, p = _update_args(src, assign, n_clusters, previous)
    return _update(_unit_rows(src, eps), a, K, p, eps)


def cluster_members(assign: torch.Tensor, n_clusters: int):
    """(offsets (K+1,), order (N,)) int64 of ``assign`` (N,) with values in [0, n_clusters): the rows of cluster k are
    ``order[offsets[k]:offsets[k+1]]`` in ascending row index."""
    if not torch.is_tensor(assign) or assign.dim() != 1 or assign.shape[0] < 1:
        raise MI355Error("assign must be a non-empty 1-D tensor")
    a = _rank._int64_on(assign, "assign", assign.shape[0], assign.device)
    if not _rank._is_int(n_clusters) or n_clusters < 1:
        raise MI355Error(f"n_clusters must be a positive integer, got {n_clusters!r}")
    N, K, dev = a.shape[0], int(n_clusters), a.device
    offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
    order = torch.empty(N, dtype=torch.int64, device=dev)
    L = lib()
    ws = _rank._ws.get(dev, L.mi355_cluster_members_workspace_bytes(N, K))
    with torch.cuda.device(dev):
        check(L.mi355_cluster_members(a.data_ptr(), N, K, offsets.data_ptr(), order.data_ptr(), ws.data_ptr(), ws.numel(),
                                      stream_ptr(dev)))
    return offsets, order


def seeded_rows(N: int, n_clusters: int, seed: int) -> np.ndarray:
    """``n_clusters`` distinct row indices in [0, N): the head of the permutation that sorts the portable generator's uniform
    stream ``seed`` (stable): the same on every machine."""
    return np.argsort(synth.uniform(int(seed), (N,)), kind="stable")[:n_clusters].astype(np.int64)


def spherical_kmeans(rows, n_clusters: int, *, iters: int = 20, seed: int = 0, init: torch.Tensor | None = None,
                     block: int | None = None, eps: float = _EPS) -> KMeansResult:
    """Spherical k-means (cosine similarity, unit centroids) of ``rows`` (a ``Gallery`` or a (N, D) fp32 device tensor).
    Starts from ``init`` (K, D), or from ``n_clusters`` distinct rows drawn by a seeded permutation (``seeded_rows``), and
    runs exactly ``assign_clusters`` then ``update_centroids`` until a pass changes no assignment (``converged``) or ``iters``
    updates are done; the returned assignments and scores are those of the returned centroids.  A raw tensor is normalised
    once into a temporary for the updates, while every assignment pass reads the raw rows and takes their norms again (one
    more pass over the rows per iteration: cluster a ``Gallery`` to avoid it).  A centroid that no update replaced comes
    back as the start gave it, not normalised.  Deterministic: the same bits for the same input, seed and start."""
    src = _rows_of(rows)
    require_cuda(src.buf, "rows")
    _check_rows(src)
    K = _check_k(n_clusters, src.rows)
    if not _rank._is_int(iters) or iters < 0:
        raise MI355Error(f"iters must be a non-negative integer, got {iters!r}")
    if init is None:
        pick = torch.from_numpy(seeded_rows(src.rows, K, seed)).to(src.device)
        c = src.data[pick].float().contiguous()
    else:
        c = _centroids_of(init, src, "init")
        if c.shape[0] != K:
            raise MI355Error(f"init must be ({K}, {src.dim}), got {tuple(c.shape)}")
    unit = _unit_rows(src, eps)
    last, members, counts = None, None, None
    passes, updates, converged = 0, 0, False
    while True:
        assign, score = _assign(src, c, block, eps)
        passes += 1
        if last is not None and torch.equal(assign, last):
            converged = True
            break
        if updates == iters:
            break
        c, counts, members = _update(unit, assign, K, c, eps)
        updates += 1
        last = assign
    if not converged:                                   # counts / members of the returned assignments
        members = cluster_members(assign, K)
        counts = members[0][1:] - members[0][:-1]
    objective = float(score.double().mean())
    if not np.isfinite(objective):
        raise MI355Error(f"spherical_kmeans: the objective is not finite ({objective}); the rows or the start hold NaN / inf")
    return KMeansResult(c, assign, score, counts, members, objective, passes, converged)


# ---- DBSCAN and threshold components: clustering without a number of clusters
class DBSCANResult(NamedTuple):
    labels: torch.Tensor          # (N,) int64: the cluster of every row, 0 .. n_clusters - 1 by ascending root; -1 = noise
    core: torch.Tensor            # (N,) bool: degree >= min_samples
    degree: torch.Tensor          # (N,) int64: rows at or above the threshold, the row itself included
    roots: torch.Tensor           # (C,) int64: each cluster's smallest core row, ascending
    counts: torch.Tensor          # (C,) int64: rows per cluster, border rows included
    n_clusters: int
    n_noise: int


_DBSCAN = {torch.float32: ("mi355_dbscan_degree", "mi355_dbscan_link", "mi355_dbscan_workspace_bytes"),
           torch.float16: ("mi355_dbscan_degree_f16", "mi355_dbscan_link_f16", "mi355_dbscan_f16_workspace_bytes")}
_DBSCAN_BLOCK = 4096              # rows per GEMM call: the fp32 copy of one block of fp16 rows stays at 4096 x D
_MAX_N_DBSCAN = (1 << 31) - 128


def dbscan(rows, threshold: float, min_samples: int = 5, *, block: int | None = None, eps: float = _EPS) -> DBSCANResult:
    """DBSCAN (Ester et al., KDD 1996) on cosine similarity, inside the tiled cosine GEMM: no number of clusters, and no
    pair list - the self-join is swept twice, ``block`` rows at a time as the queries, first counting every row's hits, then
    joining core rows in a lock-free union-find on the GPU (the hooking rule of Jaiganesh & Burtscher, HPDC 2018).

    ``hit(i, j)``: the score of row i as a query against row j is ``>= threshold`` - the score bits and the comparison of
    this gallery's own ``range_search`` of its rows (NaN never hits), row i itself included.  ``degree[i]`` counts the hits of
    row i (itself too, as sklearn counts); row i is a core row when ``degree[i] >= min_samples``.  Core rows i, j are linked
    when ``hit(i, j)`` or ``hit(j, i)``; the clusters are the connected components of the core rows, each named by its root,
    its smallest core row, and numbered 0 .. C-1 by ascending root.  A non-core row joins the cluster of the core row that
    hits it (or that it hits) with the highest score, equal scores going to the lower core row - sklearn gives such a border
    row to whichever cluster reaches it first; here the choice depends on the rows alone.  A non-core row without such a core
    row is noise, label -1.  With ``min_samples=1`` this is exactly ``connected_components``.

    ``rows``: a ``Gallery`` (fp32 or fp16, read where it lies; a prepared one on its fp32 rows) or a (N, D) fp32 device
    tensor, which is normalised once into a temporary (N x D fp32) and clustered as an fp32 ``Gallery`` of it would be.
    ``block`` (default 4096) never changes the result, nor does anything else but the rows: the same bits on every run.
    One host sync (the dense numbering).  ``clustering_metrics(result.labels, labels)`` counts the noise rows, label -1, as
    one more cluster."""
    src = _rows_of(rows)
    require_cuda(src.buf, "rows")
    t = _rank._range_threshold(threshold)
    if not _rank._is_int(min_samples) or min_samples < 1:
        raise MI355Error(f"min_samples must be an integer >= 1, got {min_samples!r}")
    if block is not None and (not _rank._is_int(block) or block < 1):
        raise MI355Error(f"block must be a positive integer, got {block!r}")
    if src.dim < 1:
        raise MI355Error(f"clustering needs at least one column, got {src.shape}")
    N, D, dev = src.rows, src.dim, src.device
    if N >= _MAX_N_DBSCAN:
        raise MI355Error(f"dbscan: {N} rows, the limit is {_MAX_N_DBSCAN - 1}")
    if N == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return DBSCANResult(e, torch.empty(0, dtype=torch.bool, device=dev), e.clone(), e.clone(), e.clone(), 0, 0)
    run = _DBSCANRun(_unit_rows(src, eps), t, int(min(min_samples, 2**31 - 1)), block, eps)
    run.sweep(link=False)
    run.sweep(link=True)
    return run.finish()


class _DBSCANRun:
    """The state and the three phases of one ``dbscan`` call on normalised rows ``src`` (tools/dbscan_bench.py times them one
    by one): ``sweep(False)`` counts the degrees, ``sweep(True)`` links, ``finish()`` resolves the roots and numbers them."""

    def __init__(self, src, threshold: float, min_samples: int, block, eps: float):
        N, dev = src.rows, src.device
        self.src, self.t, self.ms, self.eps = src, threshold, min_samples, eps
        self.block = min(_DBSCAN_BLOCK if block is None else int(block), N)
        self.degree = torch.empty(N, dtype=torch.int32, device=dev)
        self.parent = torch.empty(N, dtype=torch.int32, device=dev)
        self.border = torch.empty(N, dtype=torch.int64, device=dev)
        self.e_degree, self.e_link, ws_bytes = _DBSCAN[src.dtype]
        self.ws = _rank._ws.get(dev, getattr(lib(), ws_bytes)(self.block, N, src.dim))
        with torch.cuda.device(dev):
            check(lib().mi355_dbscan_init(N, self.degree.data_ptr(), self.parent.data_ptr(), self.border.data_ptr(), stream_ptr(dev)))

    def sweep(self, link: bool) -> None:
        src, L = self.src, lib()
        entry = getattr(L, self.e_link if link else self.e_degree)
        state = (self.ms, self.degree.data_ptr(), self.parent.data_ptr(), self.border.data_ptr()) if link else (self.degree.data_ptr(),)
        data = src.data
        with torch.cuda.device(src.device):
            for q0 in range(0, src.rows, self.block):
                q = data[q0: q0 + self.block].float().contiguous()      # fp32 rows: the rows themselves, no copy
                check(entry(q.data_ptr(), q0, q.shape[0], *src.c_args(), self.eps, self.t, *state, self.ws.data_ptr(),
                            self.ws.numel(), stream_ptr(src.device)))

    def finish(self) -> DBSCANResult:
        N, dev = self.src.rows, self.src.device
        root = torch.empty(N, dtype=torch.int64, device=dev)
        core = torch.empty(N, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib().mi355_dbscan_finish(N, self.ms, self.degree.data_ptr(), self.parent.data_ptr(), self.border.data_ptr(),
                                            root.data_ptr(), core.data_ptr(), stream_ptr(dev)))
        member = root >= 0
        roots, inverse, counts = torch.unique(root[member], sorted=True, return_inverse=True, return_counts=True)
        labels = torch.full((N,), -1, dtype=torch.int64, device=dev)
        labels[member] = inverse
        return DBSCANResult(labels, core.bool(), self.degree.long(), roots, counts, int(roots.shape[0]), N - int(inverse.shape[0]))


def connected_components(rows, threshold: float, **kw) -> DBSCANResult:
    """The connected components of the threshold graph of ``rows`` (rows i, j joined when ``hit(i, j)`` or ``hit(j, i)``, see
    ``dbscan``): ``dbscan(rows, threshold, min_samples=1, **kw)`` - every row is a core row, no row is noise, and a
    component's root is its smallest row.  The de-duplication groups of ``range_search`` pairs, without the pairs."""
    return dbscan(rows, threshold, 1, **kw)


def _dense(t, name: str):
    if not torch.is_tensor(t):
        raise MI355Error(f"{name} must be a tensor")
    require_cuda(t, name)
    if t.dim() != 1 or t.shape[0] < 1:
        raise MI355Error(f"{name} must be a non-empty 1-D tensor, got {tuple(t.shape)}")
    t = _rank._int64_on(t, name, t.shape[0], t.device)
    values, inverse = torch.unique(t, sorted=True, return_inverse=True)
    return values, inverse.contiguous()


def contingency(a: torch.Tensor, b: torch.Tensor):
    """(table (Ka, Kb) int64, a_values (Ka,), b_values (Kb,)): ``table[i, j]`` = the positions where ``a == a_values[i]`` and
    ``b == b_values[j]``; the labels (any int64 values) are made dense by sorted unique value.  Exact integer counts."""
    av, ai = _dense(a, "a")
    bv, bi = _dense(b, "b")
    if ai.shape[0] != bi.shape[0] or ai.device != bi.device:
        raise MI355Error(f"a and b must have one length and one device, got {tuple(a.shape)} on {a.device} and "
                         f"{tuple(b.shape)} on {b.device}")
    N, Ka, Kb, dev = ai.shape[0], av.shape[0], bv.shape[0], ai.device
    if Ka * Kb > 1 << 28:
        raise MI355Error(f"contingency table too large: {Ka} x {Kb} > 2^28 cells")
    table = torch.empty((Ka, Kb), dtype=torch.int64, device=dev)
    L = lib()
    ws = _rank._ws.get(dev, L.mi355_contingency_workspace_bytes(N, Ka, Kb))
    with torch.cuda.device(dev):
        check(L.mi355_contingency(ai.data_ptr(), bi.data_ptr(), N, Ka, Kb, table.data_ptr(), ws.data_ptr(), ws.numel(),
                                  stream_ptr(dev)))
    return table, av, bv


def _pairs(x: np.ndarray) -> float:
    x = x.astype(np.float64)
    return float((x * (x - 1.0) / 2.0).sum())


def clustering_metrics_from_table(table) -> dict:
    """The scores of a contingency table n_ij (rows: clusters, columns: classes), host float64, no GPU.  With a_i / b_j the
    row / column sums and N the total: I = sum (n_ij/N) ln(N n_ij / (a_i b_j)) over non-zero cells, ``nmi`` = 2I / (H(a) + H(b))
    (1 when both entropies are 0), ``purity`` = sum_i max_j n_ij / N, TP = sum C(n_ij, 2), ``precision`` = TP / sum C(a_i, 2),
    ``recall`` = TP / sum C(b_j, 2) (0/0 counts as 1), ``f1`` their harmonic mean."""
    if torch.is_tensor(table):
        table = table.detach().cpu().numpy()
    n = np.asarray(table)
    if n.ndim != 2 or n.size == 0 or not np.issubdtype(n.dtype, np.integer) or (n < 0).any() or n.sum() < 1:
        raise MI355Error("the contingency table must be a non-empty 2-D array of non-negative integer counts, not all zero")
    n = n.astype(np.float64)
    N = n.sum()
    a, b = n.sum(axis=1), n.sum(axis=0)
    i, j = np.nonzero(n)
    nz = n[i, j]
    info = float((nz / N * np.log(N * nz / (a[i] * b[j]))).sum())

    def entropy(m):
        m = m[m > 0]
        return float(-(m / N * np.log(m / N)).sum())

    h = entropy(a) + entropy(b)
    tp, pa, pb = _pairs(n), _pairs(a), _pairs(b)
    precision = tp / pa if pa > 0 else 1.0
    recall = tp / pb if pb > 0 else 1.0
    f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return {"nmi": 2.0 * info / h if h > 0 else 1.0, "purity": float(n.max(axis=1).sum() / N), "f1": f1,
            "precision": precision, "recall": recall, "n_clusters": int((a > 0).sum()), "n_classes": int((b > 0).sum())}


def clustering_metrics(assignments: torch.Tensor, labels: torch.Tensor) -> dict:
    """``nmi``, ``purity``, ``f1``, ``precision``, ``recall``, ``n_clusters``, ``n_classes`` of cluster ``assignments`` (N,)
    against class ``labels`` (N,) (device integer tensors, any values): the contingency table on the GPU, the scores of
    ``clustering_metrics_from_table`` on the host."""
    return clustering_metrics_from_table(contingency(assignments, labels)[0])
