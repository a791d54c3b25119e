"""Inverted-file (IVF) search over a resident ``Gallery``: the centroids of a spherical k-means are the coarse quantiser, the
members of every cluster are its lists, and a query is scored against the rows of the ``nprobe`` lists nearest to it only.

* ``IVFIndex(gallery, centroids, assignments)`` .. the lists of given assignments (CSR from ``cluster_members``)
* ``IVFIndex.build(gallery, nlist)`` ............. ``gallery.kmeans(nlist)``, then the constructor (``Gallery.ivf`` caches it)
* ``index.probe(queries, nprobe)`` ............... the nearest lists: the fp32 top-k of the queries against the centroids
* ``index.search(queries, k, nprobe)`` ........... scan of the probed lists (``mi355_ivf_scan``), ``merge_topk``, ``clear_pads``
* ``index.recall(queries, k, nprobe)`` ........... the share of the exhaustive top-k it returns: how to choose ``nprobe``
* ``index.update()`` ............................. after ``gallery.add``: the new rows go to their nearest list

The rows are scanned where they lie in the gallery (fp32 or fp16), through the lists' ``order``; the index holds no copy of
them.  The lists, ``probe``, ``stale``, the rules for ``nprobe`` / ``probes`` and the search around the scan are
``_lists._ListIndex``, shared with every list index.  The scan itself - the query blocks, the candidate slab of one block, its
``merge_topk`` and ``clear_pads`` - is ``_SlabIndex`` here, shared with ``Int8IVFIndex`` (ivf_i8.py): a class names its two C
entries and its row arguments.  Out of scope: ``ShardedGallery``, a list-ordered copy of the rows.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr
from ._lists import _ListIndex
from .rank import _is_int

_SLAB_BYTES = 256 << 20             # the candidate slab of one query block (12 B per slot) stays under this


class _SlabIndex(_ListIndex):
    """A list index over rows that are scanned where they lie in the store: a block of queries fills a candidate slab, of which
    ``merge_topk`` keeps the best."""

    _ENTRIES = ()                           # the C entries: the workspace sizer and the scan
    # a subclass also has ``_row_args()``: what the scan entry takes between ``eps`` and the row stride

    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        q = _rank._f32c(queries, "queries")
        _rank._check_qg(q, self._store._resident())
        return q

    def _block(self, Q: int, nprobe: int, cap: int, block) -> int:
        if block is not None:
            if not _is_int(block) or block < 1:
                raise MI355Error(f"block must be a positive integer, got {block!r}")
            return int(block)
        return max(1, min(_SLAB_BYTES // (12 * cap), ((1 << 31) - 1) // nprobe, 65535 * 16))

    def _scan(self, q, probes, cap, idx_offset, filt):
        """The candidate slab (values (n, cap) fp32, indices (n, cap) int64) of the queries ``q`` (n, D) probing ``probes``."""
        g, L = self._store, lib()
        sizer, scan = self._ENTRIES
        n, nprobe, dev = q.shape[0], probes.shape[1], q.device
        cand_val = torch.empty((n, cap), dtype=torch.float32, device=dev)
        cand_idx = torch.empty((n, cap), dtype=torch.int64, device=dev)
        ws = _rank._ws.get(dev, getattr(L, sizer)(n, nprobe, self.nlist, g.dim, cap))
        with torch.cuda.device(dev):
            check(getattr(L, scan)(q.data_ptr(), n, g.dim, g.eps, *self._row_args(), g._ld, g.rows, self.offsets.data_ptr(),
                                   self.order.data_ptr(), self.nlist, probes.data_ptr(), nprobe, cap, int(idx_offset),
                                   None if filt is None else filt[0], cand_val.data_ptr(), cand_idx.data_ptr(), ws.data_ptr(),
                                   ws.numel(), stream_ptr(dev)))
        return cand_val, cand_idx

    def _top_of_lists(self, q, probes, cap, R, idx_offset, filt, block):
        Q, rows = q.shape[0], self._store.rows
        blk = self._block(Q, probes.shape[1], cap, block)
        vals = torch.empty((Q, R), dtype=torch.float32, device=q.device)
        idx = torch.empty((Q, R), dtype=torch.int64, device=q.device)
        for q0 in range(0, Q, blk):
            q1 = min(Q, q0 + blk)
            cand_val, cand_idx = self._scan(q[q0:q1], probes[q0:q1].contiguous(), cap, idx_offset, _rank._filter_from(filt, q0))
            v, i = _rank.merge_topk(cand_val, cand_idx, R)
            _rank.clear_pads(v, i, int(idx_offset), int(idx_offset) + rows)
            vals[q0:q1], idx[q0:q1] = v, i
        return vals, idx


class IVFIndex(_SlabIndex):
    """The lists of a ``Gallery``: ``centroids`` (nlist, D) fp32, ``offsets`` (nlist + 1,) / ``order`` (rows,) int64 (the rows
    of list l are ``order[offsets[l]:offsets[l + 1]]``, ascending), ``counts`` (nlist,) int64, and a reference to the gallery."""

    _STORE, _NOUN, _STORE_NOUN, _HINT = "gallery", "IVF index", "gallery", "call update()"
    _ENTRIES = ("mi355_ivf_scan_workspace_bytes", "mi355_ivf_scan")

    def __init__(self, gallery, centroids: torch.Tensor, assignments: torch.Tensor):
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"an IVF index is built over a Gallery, got {type(gallery).__name__}")
        if gallery.rows < 1:
            raise MI355Error("an IVF index needs a gallery with at least one row")
        self.gallery = gallery
        self._init_lists(_cl._centroids_of(centroids, gallery._resident()), assignments)

    @classmethod
    def build(cls, gallery, nlist: int, *, iters: int = 10, seed: int = 0, init: torch.Tensor | None = None) -> "IVFIndex":
        """``gallery.kmeans(nlist, iters=, seed=, init=)``, then the lists of its assignments."""
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"an IVF index is built over a Gallery, got {type(gallery).__name__}")
        r = gallery.kmeans(nlist, iters=iters, seed=seed, init=init)
        return cls(gallery, r.centroids, r.assignments)

    def update(self) -> "IVFIndex":
        """After ``gallery.add`` (the index is ``stale``): ``assign_clusters`` of the new rows only against the unchanged
        centroids, then the CSR again."""
        g = self.gallery
        if g.rows < self.rows:
            raise MI355Error(f"the gallery has {g.rows} rows but the index lists {self.rows}")
        if g.rows > self.rows:
            new = _rank._Rows(g._buf[self.rows: g.rows], g.rows - self.rows, g.dim, True)
            a, _ = _cl.assign_clusters(new, self.centroids, eps=g.eps)
            self._set_lists(torch.cat([self.assignments, a]))
        return self

    def _row_args(self):
        return self.gallery._buf.data_ptr(), _rank._DTYPES[self.gallery.dtype]

    def search(self, queries: torch.Tensor, k: int, nprobe: int | None = None, *, probes: torch.Tensor | None = None,
               query_labels: torch.Tensor | None = None, label_filter: str | None = None,
               exclude: torch.Tensor | None = None, idx_offset: int = 0, block: int | None = None):
        """(values (Q, k) fp32, indices (Q, k) int64): the top-k of the rows of every query's probed lists, ordered as
        ``Gallery.search`` orders them (descending, ties to the lower index).  Exactly one of ``nprobe`` (the lists of
        ``probe(queries, nprobe)``) and ``probes`` ((Q, n) int64 list ids, distinct within a row) is given.  A score is
        ``qn . row`` in fp32 (fp16 rows widened exactly) and depends on its query and its row only: not on the other queries,
        ``nprobe`` or ``block``.  Filters and ``idx_offset`` as in ``Gallery.search``; with fewer than k eligible probed rows
        the remaining slots are (-inf, -1).  ``1 <= k <= min(1024, rows)``.  The queries go through ``block`` at a time
        (default: what keeps the candidate slab under 256 MB); the result does not depend on it."""
        return self._search_lists(queries, k, nprobe, probes, query_labels, label_filter, exclude, idx_offset, block=block)

    def recall(self, queries: torch.Tensor, k: int, nprobe: int):
        """(mean, per_query (Q,) float64): the share of ``gallery.search(queries, k)``'s indices that
        ``search(queries, k, nprobe)`` returns."""
        return self._recall_lists(queries, k, nprobe, None)
