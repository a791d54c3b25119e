"""IVF-PQ search: inverted-file lists over the codes of a ``PQGallery``.  The centroids of a spherical k-means of the rows the
codes were made from are the coarse quantiser; a query pays table lookups only for the rows of the ``nprobe`` lists nearest to
it, not for every row of the gallery as ``PQGallery.search`` does.

* ``IVFPQIndex(pq, centroids, assignments)`` ......... the lists of given assignments over ``pq``'s rows
* ``IVFPQIndex.build(pq, rows, nlist)`` .............. ``spherical_kmeans`` of ``rows`` (the ``Gallery`` or the fp32 tensor the
  codes were made from), then the constructor (``PQGallery.ivf`` is the same)
* ``IVFPQIndex.from_gallery(gallery, M, nlist)`` ..... ``PQGallery.from_gallery``, then ``build``
* ``index.probe(queries, nprobe)`` ................... the nearest lists: the fp32 top-k of the queries against the centroids
* ``index.search(queries, k, nprobe, refine=None)`` .. scan of the probed lists' codes (``mi355_ivfpq_search``)
* ``index.recall(queries, k, nprobe, exact=None)`` ... against ``pq.search`` (what the lists lose) or a ``Gallery``
* ``index.add(embeddings, labels=None)`` ............. ``pq.add``, the new rows to their nearest lists, the lists again

The index codes nothing itself: a score is the PQ score of the gallery's own code row, bit for bit, so a search that probes
every list returns exactly what ``pq.search`` returns.  It keeps a list-ordered copy of the codes (``list_codes[p] =
pq.codes[order[p]]``, M bytes per row): every list is one contiguous byte range, which is what the scan reads; ``pq.codes``
stays the record.  The lists, ``probe``, ``stale``, ``add``, ``recall``, the rules for ``nprobe`` / ``probes`` and the search
around the scan are ``_lists._ListIndex``, shared with every list index; ``_scan`` here is the one call of the code scan.
Residual codes (a row's offset from its list centroid) are ``ResidualIVFPQIndex`` (ivfrpq.py), which names two other C entries
and adds its centroids to the call.  Out of scope: an OPQ rotation, an index over a sharded PQ gallery.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import pq as _pq
from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr
from ._lists import _check_rows, _ListIndex

SCAN_CHUNK = 2048                   # positions of one scan workgroup (IVFPQ_CHUNK, csrc/ivfpq.hip)


def _check_pq(pq) -> None:
    if not isinstance(pq, _pq.PQGallery):
        raise MI355Error(f"an IVF-PQ index is built over a PQGallery, got {type(pq).__name__}")
    pq._trained("IVFPQIndex")
    if pq.rows < 1:
        raise MI355Error("an IVF-PQ index needs a PQGallery with at least one row")


class IVFPQIndex(_ListIndex):
    """The lists of a ``PQGallery``: ``centroids`` (nlist, D) fp32, ``assignments`` (rows,), ``offsets`` (nlist + 1,) / ``order``
    (rows,) int64 (the rows of list l are ``order[offsets[l]:offsets[l + 1]]``, ascending), ``counts`` (nlist,) int64,
    ``list_codes`` (rows, M) uint8 (the codes in list order) and a reference to ``pq``.  ``stale``: rows were added to ``pq``
    behind the index's back (``index.add`` keeps the two together)."""

    _STORE, _NOUN, _STORE_NOUN = "pq", "IVF-PQ index", "PQGallery"
    _HINT = "add rows through index.add, or build the index again"
    _EXTRA = ("list_codes",)
    _ENTRIES = ("mi355_ivfpq_search_workspace_bytes", "mi355_ivfpq_search")     # the C entries: the workspace sizer and the scan
    list_codes = None
    add = _ListIndex._add_to_store

    def __init__(self, pq, centroids: torch.Tensor, assignments: torch.Tensor):
        _check_pq(pq)
        self.pq = pq
        self._init_lists(self._checked_centroids(centroids), assignments)

    def _relist(self) -> None:
        _rank._retire(self.list_codes, self.pq.device)               # a queued search may still read the old copy
        self.list_codes = self.pq.codes.index_select(0, self.order)

    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        return self.pq._queries(queries, "search")

    @classmethod
    def build(cls, pq, rows, nlist: int, *, iters: int = 10, seed: int = 0, init: torch.Tensor | None = None) -> "IVFPQIndex":
        """``spherical_kmeans(rows, nlist, iters=, seed=, init=)``, then the lists of its assignments over ``pq``'s rows.
        ``rows`` is the fp32 / fp16 ``Gallery``, or the (N, D) fp32 tensor, the codes were made from."""
        _check_pq(pq)
        _check_rows(pq, rows)
        r = _cl.spherical_kmeans(rows, nlist, iters=iters, seed=seed, init=init, eps=pq.eps)
        return cls(pq, r.centroids, r.assignments)

    @classmethod
    def from_gallery(cls, gallery, M: int, nlist: int, *, pq_iters: int = 10, iters: int = 10, seed: int = 0) -> "IVFPQIndex":
        """``PQGallery.from_gallery(gallery, M, pq_iters, seed)``, then ``build`` over the same rows."""
        pq = _pq.PQGallery.from_gallery(gallery, M, iters=pq_iters, seed=seed)
        return cls.build(pq, gallery, nlist, iters=iters, seed=seed)

    def _scan_args(self):
        """What the scan entry takes between the filter and the outputs."""
        return ()

    def _scan(self, q, probes, cap, k, idx_offset, filt):
        """(values (Q, k) fp32, indices (Q, k) int64): the top-k of the codes of the lists ``probes`` (Q, nprobe) names."""
        pq, dev, L = self.pq, self.pq.device, lib()
        sizer, scan = self._ENTRIES
        Q, nprobe = q.shape[0], probes.shape[1]
        vals = torch.empty((Q, k), dtype=torch.float32, device=dev)
        idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
        if Q:
            ws = _rank._ws.get(dev, getattr(L, sizer)(Q, nprobe, self.nlist, pq.dim, pq.M, cap, k))
            with torch.cuda.device(dev):
                check(getattr(L, scan)(q.data_ptr(), Q, pq.dim, pq.eps, pq._codebooks.data_ptr(), pq.M, self.list_codes.data_ptr(),
                                       self.rows, self.offsets.data_ptr(), self.order.data_ptr(), self.nlist, probes.data_ptr(),
                                       nprobe, cap, k, int(idx_offset), None if filt is None else filt[0], *self._scan_args(),
                                       vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(dev)))
        return vals, idx

    def _top_of_lists(self, q, probes, cap, R, idx_offset, filt, block):
        return self._scan(q, probes.contiguous(), cap, R, idx_offset, filt)

    def search(self, queries: torch.Tensor, k: int, nprobe: int | None = None, *, probes: torch.Tensor | None = None,
               query_labels: torch.Tensor | None = None, label_filter: str | None = None, exclude: torch.Tensor | None = None,
               idx_offset: int = 0, refine=None, shortlist: int | None = None):
        """(values (Q, k) fp32, indices (Q, k) int64): the top-k of the rows of every query's probed lists, scored and ordered
        as ``PQGallery.search`` scores and orders them (descending, ties to the lower gallery row).  Exactly one of ``nprobe``
        (the lists of ``probe(queries, nprobe)``) and ``probes`` ((Q, n) int64 list ids, distinct within a row) is given.
        Filters, ``idx_offset``, ``refine`` and ``shortlist`` as in ``PQGallery.search`` (the shortlist comes from the probed
        lists).  With fewer than k eligible probed rows the remaining slots are (-inf, -1).  ``1 <= k <= min(1024, rows)``.
        Probing every list returns ``pq.search``'s result bit for bit.  The scan's flags are read back once, at the end (a host sync on
        the current stream): bad lists raise."""
        return self._search_lists(queries, k, nprobe, probes, query_labels, label_filter, exclude, idx_offset, refine, shortlist)

    def recall(self, queries: torch.Tensor, k: int, nprobe: int, exact=None, **search_kwargs):
        """(mean, per_query (Q,) float64): the share of the reference's top-k indices that ``search(queries, k, nprobe,
        **search_kwargs)`` returns.  ``exact=None``: the reference is ``pq.search(queries, k)`` - what the lists lose.  A
        ``Gallery`` of the same rows: its exact search - what lists and codes lose together."""
        return self._recall_lists(queries, k, nprobe, exact, **search_kwargs)
