"""Graph search over a resident ``Gallery``: a beam walk (best-first search) over the gallery's exact kNN graph, started at the
rows nearest the centroids of a spherical k-means.

* ``merged_graph(fwd, degree)`` ................. the (G, degree) int32 adjacency of (G, degree // 2) forward lists: the forward
  neighbours, then the reverse neighbours that are not forward ones
* ``GraphIndex(gallery, graph, entries, centroids)`` .. an index of hand-made parts
* ``GraphIndex.build(gallery, nentry)`` ......... ``gallery.knn_graph(degree // 2)`` merged, ``gallery.kmeans(nentry)``, and the
  row nearest every centroid as its entry point (``Gallery.graph`` caches it)
* ``index.seeds(queries, nseed)`` ............... the entry points of the ``nseed`` centroids nearest every query
* ``index.search(queries, k, ef, nseed)`` ....... the walk (``mi355_graph_search``): one workgroup per query
* ``index.recall(queries, k, ef, nseed)`` ....... the share of the exhaustive top-k it returns: how to choose ``ef``

The rows are read where they lie in the gallery (fp32 or fp16); the index holds the graph, the entry points and the centroids.
The result is approximate against ``Gallery.search`` but a pure function of the rows, the graph, the seeds and (k, ef,
max_iters): include/mi355_retrieval.h states it step by step.  Any ``gallery.add`` makes the index stale.  Out of scope:
incremental insert, edge pruning, int8 / PQ rows, a sharded graph.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import rank as _rank
from ._lib import MI355Error, check, lib, require_cuda, stream_ptr
from .rank import _is_int

MAX_EF, MAX_DEGREE, MAX_NSEED, MAX_VISITS, MAX_DIM = 512, 64, 64, 16384, 4096
_DEDUP_ROWS = 1 << 16               # rows of one block of the duplicate mask (block x h x h booleans)


def _check_degree(degree) -> int:
    if not _is_int(degree) or degree % 2 or not 2 <= degree <= MAX_DEGREE:
        raise MI355Error(f"degree={degree!r} must be an even integer in [2, {MAX_DEGREE}]")
    return int(degree)


def merged_graph(fwd: torch.Tensor, degree: int) -> torch.Tensor:
    """The (G, degree) int32 adjacency of the forward lists ``fwd`` (G, degree // 2) integer (row ids; a negative entry is a
    pad).  Slots [0, h) of row r are ``fwd[r]`` as given; slots [h, degree) are the reverse neighbours of r - the rows s with r
    in ``fwd[s]`` that are not in ``fwd[r]`` already - ordered by (the first position of r in ``fwd[s]``, s) and cut to
    ``degree - h``; the slots left over hold -1.  Stable torch sorts on the tensor's device: the same bits every time."""
    degree = _check_degree(degree)
    h = degree // 2
    if not torch.is_tensor(fwd) or fwd.dim() != 2 or fwd.shape[1] != h:
        raise MI355Error(f"fwd must be a (G, degree // 2 = {h}) tensor")
    if fwd.dtype.is_floating_point or fwd.dtype.is_complex or fwd.dtype == torch.bool:
        raise MI355Error(f"fwd must hold integers, got {fwd.dtype}")
    G, dev = int(fwd.shape[0]), fwd.device
    if G >= 1 << 31:
        raise MI355Error(f"G={G} must be below 2^31")
    f = fwd.to(torch.int64)
    out = torch.full((G, degree), -1, dtype=torch.int32, device=dev)
    out[:, :h] = f.to(torch.int32)
    if G == 0:
        return out
    # an edge s -> r counts once, at the first position of r in fwd[s]
    edge = (f >= 0) & (f < G)
    earlier = torch.ones((h, h), dtype=torch.bool, device=dev).tril(-1)                      # [j][i]: i < j
    for r0 in range(0, G, _DEDUP_ROWS):
        b = f[r0: r0 + _DEDUP_ROWS]
        edge[r0: r0 + _DEDUP_ROWS] &= ~((b.unsqueeze(2) == b.unsqueeze(1)) & earlier).any(dim=2)
    src = torch.arange(G, dtype=torch.int64, device=dev).unsqueeze(1).expand(G, h)
    # in the order (position, s); what is a forward neighbour of its target already is no reverse neighbour
    dst, s, keep = f.t().reshape(-1), src.t().reshape(-1), edge.t().reshape(-1)
    fkeys = (src * G + f)[edge]                                                              # r * G + n: n is in fwd[r]
    keep = keep & ~torch.isin(dst * G + s, fkeys)
    dst, s = dst[keep], s[keep]
    dst, perm = torch.sort(dst, stable=True)                                                 # by target, (position, s) within it
    s = s[perm]
    counts = torch.bincount(dst, minlength=G)
    rank = torch.arange(dst.shape[0], dtype=torch.int64, device=dev) - (torch.cumsum(counts, 0) - counts)[dst]
    fits = rank < degree - h
    out[dst[fits], h + rank[fits]] = s[fits].to(torch.int32)
    return out


class GraphIndex:
    """``graph`` (rows, degree) int32 (row r lists the neighbours of r, -1 a pad), ``entries`` (nentry,) int64 rows,
    ``centroids`` (nentry, D) fp32 - entry point c is the row a search starts from when centroid c is near the query - and a
    reference to the gallery."""

    def __init__(self, gallery, graph: torch.Tensor, entries: torch.Tensor, centroids: torch.Tensor):
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"a graph index is built over a Gallery, got {type(gallery).__name__}")
        if gallery.rows < 1:
            raise MI355Error("a graph index needs a gallery with at least one row")
        if not torch.is_tensor(graph) or graph.dim() != 2 or graph.dtype != torch.int32:
            raise MI355Error("graph must be a (rows, degree) int32 tensor")
        if graph.shape[0] != gallery.rows or not 2 <= graph.shape[1] <= MAX_DEGREE:
            raise MI355Error(f"graph must be (rows={gallery.rows}, degree in [2, {MAX_DEGREE}]), got {tuple(graph.shape)}")
        require_cuda(graph, "graph")
        if graph.device != gallery.device:
            raise MI355Error(f"graph is on {graph.device} but the gallery on {gallery.device}")
        self.gallery = gallery
        self.centroids = _cl._centroids_of(centroids, gallery._resident())
        self.nentry = int(self.centroids.shape[0])
        self.entries = _rank._int64_on(entries, "entries", self.nentry, gallery.device)
        self.graph = graph.contiguous()
        self.degree = int(graph.shape[1])
        self.rows = int(gallery.rows)

    @classmethod
    def build(cls, gallery, nentry: int, *, degree: int = 32, iters: int = 10, seed: int = 0,
              init: torch.Tensor | None = None) -> "GraphIndex":
        """The merged kNN graph of ``gallery.knn_graph(degree // 2)``, the centroids of ``gallery.kmeans(nentry, iters=, seed=,
        init=)`` and, as entry point c, the row nearest centroid c (``gallery.search(centroids, 1)``)."""
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"a graph index is built over a Gallery, got {type(gallery).__name__}")
        degree = _check_degree(degree)
        if gallery.rows <= degree // 2:
            raise MI355Error(f"a graph of degree {degree} needs more than {degree // 2} rows, the gallery holds {gallery.rows}")
        cent = gallery.kmeans(nentry, iters=iters, seed=seed, init=init).centroids
        graph = merged_graph(gallery.knn_graph(degree // 2)[1], degree)
        return cls(gallery, graph, gallery.search(cent, 1)[1].reshape(-1), cent)

    @property
    def nbytes(self) -> int:
        """The index's size in bytes: graph, entries and centroids; the rows belong to the gallery."""
        return sum(t.numel() * t.element_size() for t in (self.graph, self.entries, self.centroids))

    @property
    def stale(self) -> bool:
        """Rows were added to the gallery since the graph was made."""
        return self.rows != self.gallery.rows

    def _fresh(self) -> None:
        if self.stale:
            raise MI355Error(f"the graph index is stale: its graph has {self.rows} rows but the gallery holds "
                             f"{self.gallery.rows} (build it again: there is no incremental insert)")

    def _check_nseed(self, nseed) -> int:
        top = min(self.nentry, MAX_NSEED)
        if not _is_int(nseed) or not 1 <= nseed <= top:
            raise MI355Error(f"nseed={nseed!r} outside [1, {top}] (min(nentry, {MAX_NSEED}))")
        return int(nseed)

    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        q = _rank._f32c(queries, "queries")
        _rank._check_qg(q, self.gallery._resident())
        return q

    def seeds(self, queries: torch.Tensor, nseed: int = 8) -> torch.Tensor:
        """(Q, nseed) int64: the entry points of the ``nseed`` centroids nearest every query, nearest first -
        ``entries[cosine_topk(queries, centroids, nseed)[1]]``.  ``1 <= nseed <= min(nentry, 64)``."""
        nseed = self._check_nseed(nseed)
        return self.entries[_rank.cosine_topk(queries, self.centroids, nseed, self.gallery.eps)[1]]

    def default_max_iters(self, ef: int, nseed: int) -> int:
        """``2 * ef`` expansions, or as many as the visited set has room for: ``nseed + max_iters * degree <= 16384``."""
        return max(1, min(2 * ef, (MAX_VISITS - nseed) // self.degree))

    def search(self, queries: torch.Tensor, k: int, ef: int = 64, nseed: int = 8, *, seeds: torch.Tensor | None = None,
               max_iters: int | None = None, query_labels: torch.Tensor | None = None, label_filter: str | None = None,
               exclude: torch.Tensor | None = None, idx_offset: int = 0, stats: bool = False):
        """(values (Q, k) fp32, indices (Q, k) int64), and with ``stats=True`` also (iters (Q,), visited (Q,)) int32: the
        first k eligible entries of every query's beam after the walk from ``seeds`` ((Q, n) int64 rows, -1 skipped; default
        ``self.seeds(queries, nseed)``) - at most ``max_iters`` expansions (default ``default_max_iters``) with a beam of ``ef``
        rows.  A score is ``qn . row`` in fp32 with the bits of ``IVFIndex.search`` for that pair; the order is that of
        ``Gallery.search`` (descending, ties to the lower index).  Filters and ``idx_offset`` as in ``Gallery.search``: they
        choose among the beam's rows and never change the walk, so a filtered search may return fewer than k rows - the
        remaining slots are (-inf, -1).  ``1 <= k <= ef <= 512``; ``nseed + max_iters * degree <= 16384``; ``dim <= 4096``."""
        self._fresh()
        if not _is_int(ef) or not 1 <= ef <= MAX_EF:
            raise MI355Error(f"ef={ef!r} outside [1, {MAX_EF}]")
        if not _is_int(k) or not 1 <= k <= ef:
            raise MI355Error(f"selected index k out of range: k={k!r} outside [1, ef={ef}] (k > ef: the beam holds ef rows)")
        if seeds is None:
            nseed = self._check_nseed(nseed)
        else:
            if not torch.is_tensor(seeds) or seeds.dim() != 2:
                raise MI355Error("seeds must be a (Q, nseed) tensor")
            nseed = int(seeds.shape[1])
            if not 1 <= nseed <= MAX_NSEED:
                raise MI355Error(f"nseed={nseed} outside [1, {MAX_NSEED}]")
        if max_iters is None:
            max_iters = self.default_max_iters(int(ef), nseed)
        if not _is_int(max_iters) or max_iters < 1:
            raise MI355Error(f"max_iters={max_iters!r} must be a positive integer")
        if nseed + max_iters * self.degree > MAX_VISITS:
            raise MI355Error(f"nseed + max_iters * degree = {nseed + max_iters * self.degree} rows may be visited, more than the "
                             f"{MAX_VISITS} the visited set holds")
        g = self.gallery
        if g.dim > MAX_DIM:
            raise MI355Error(f"dim={g.dim} outside [1, {MAX_DIM}]")
        q = self._queries(queries)
        Q, dev = q.shape[0], q.device
        if seeds is None:
            seeds = self.seeds(q, nseed) if Q else torch.empty((0, nseed), dtype=torch.int64, device=dev)
        elif seeds.shape[0] != Q:
            raise MI355Error(f"seeds must be a (Q={Q}, nseed) tensor, got {tuple(seeds.shape)}")
        seeds = _rank._int64_on(seeds.reshape(-1), "seeds", Q * nseed, dev).view(Q, nseed)
        gl = None if label_filter is None else g._labels_for(f'label_filter="{label_filter}"')
        filt = _rank._rank_filter(Q, g.rows, dev, query_labels, gl, label_filter, exclude)
        vals = torch.empty((Q, k), dtype=torch.float32, device=dev)
        idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
        iters = torch.empty((Q,), dtype=torch.int32, device=dev)
        visited = torch.empty((Q,), dtype=torch.int32, device=dev)
        if Q:
            L = lib()
            ws = _rank._ws.get(dev, L.mi355_graph_search_workspace_bytes(Q, g.dim, nseed, int(ef), self.degree, int(max_iters)))
            with torch.cuda.device(dev):
                check(L.mi355_graph_search(q.data_ptr(), Q, g.dim, g.eps, g._buf.data_ptr(), _rank._DTYPES[g.dtype], g._ld, g.rows,
                                           self.graph.data_ptr(), self.degree, seeds.data_ptr(), nseed, int(k), int(ef),
                                           int(max_iters), int(idx_offset), None if filt is None else filt[0], vals.data_ptr(),
                                           idx.data_ptr(), iters.data_ptr(), visited.data_ptr(), ws.data_ptr(), ws.numel(),
                                           stream_ptr(dev)))
        return (vals, idx, iters, visited) if stats else (vals, idx)

    def recall(self, queries: torch.Tensor, k: int, ef: int = 64, nseed: int = 8):
        """(mean, per_query (Q,) float64): the share of ``gallery.search(queries, k)``'s indices that
        ``search(queries, k, ef, nseed)`` returns."""
        got = self.search(queries, k, ef, nseed)[1]
        return _rank._recall(got, self.gallery.search(queries, k)[1], k)
