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
stays the record.  The lists, ``probe``, ``stale`` and the rules for ``nprobe`` / ``probes`` are ``_lists._ListIndex``, shared
with ``IVFIndex``.  Residual codes (a row's offset from its list centroid) are ``ResidualIVFPQIndex`` (ivfrpq.py).  Out of
scope: an OPQ rotation, an index over a sharded PQ gallery.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import pq as _pq
from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr
from ._lists import _ListIndex

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
    list_codes = None

    def __init__(self, pq, centroids: torch.Tensor, assignments: torch.Tensor):
        _check_pq(pq)
        self.pq = pq
        if not torch.is_tensor(centroids):
            raise MI355Error(f"centroids must be a tensor, got {type(centroids).__name__}")
        c = centroids
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != pq.dim or c.device != pq.device:
            raise MI355Error(f"centroids must be (nlist, {pq.dim}) on {pq.device}, got {tuple(c.shape)} on {c.device}")
        self._init_lists(_rank._f32c(c, "centroids"), assignments)

    def _relist(self) -> None:
        _rank._retire(self.list_codes, self.pq.device)               # a queued search may still read the old copy
        self.list_codes = self.pq.codes.index_select(0, self.order)

    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        return self.pq._queries(queries, "search")

    @staticmethod
    def _check_rows(pq, rows) -> None:
        """``rows``: what ``pq``'s codes were made from - a Gallery (fp32 or fp16) or a (N, D) fp32 tensor, same device and dim,
        N == len(pq).  ``pq``: a ``PQGallery``, or any row store with a ``_NOUN`` (``Int8IVFIndex`` checks its rows here)."""
        if isinstance(rows, _rank.Gallery):
            n, dim, dev = len(rows), rows.dim, rows.device
        elif torch.is_tensor(rows):
            if rows.dtype != torch.float32:
                raise MI355Error(f"rows must be fp32, got {rows.dtype} (an fp16 Gallery is accepted; fp16 tensors are not)")
            if rows.dim() != 2:
                raise MI355Error(f"rows must be (N, {pq.dim}), got {tuple(rows.shape)}")
            n, dim, dev = int(rows.shape[0]), int(rows.shape[1]), rows.device
        else:
            raise MI355Error(f"rows must be a Gallery or a tensor, got {type(rows).__name__}")
        if dev != pq.device:
            raise MI355Error(f"rows are on {dev} but the {pq._NOUN} lives on {pq.device}")
        if dim != pq.dim:
            raise MI355Error(f"rows have dim {dim}, the {pq._NOUN} {pq.dim}")
        if n != pq.rows:
            raise MI355Error(f"rows holds {n} rows, the {pq._NOUN} {pq.rows}: the lists are made of the rows the codes were made from")

    @classmethod
    def build(cls, pq, rows, nlist: int, *, iters: int = 10, seed: int = 0, init: torch.Tensor | None = None) -> "IVFPQIndex":
        """``spherical_kmeans(rows, nlist, iters=, seed=, init=)``, then the lists of its assignments over ``pq``'s rows.
        ``rows`` is the fp32 / fp16 ``Gallery``, or the (N, D) fp32 tensor, the codes were made from."""
        _check_pq(pq)
        cls._check_rows(pq, rows)
        r = _cl.spherical_kmeans(rows, nlist, iters=iters, seed=seed, init=init, eps=pq.eps)
        return cls(pq, r.centroids, r.assignments)

    @classmethod
    def from_gallery(cls, gallery, M: int, nlist: int, *, pq_iters: int = 10, iters: int = 10, seed: int = 0) -> "IVFPQIndex":
        """``PQGallery.from_gallery(gallery, M, pq_iters, seed)``, then ``build`` over the same rows."""
        pq = _pq.PQGallery.from_gallery(gallery, M, iters=pq_iters, seed=seed)
        return cls.build(pq, gallery, nlist, iters=iters, seed=seed)

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None) -> "IVFPQIndex":
        """``pq.add(embeddings, labels)``, then ``assign_clusters`` of the new rows against the unchanged centroids, then the
        lists and ``list_codes`` again."""
        self._fresh()
        self.pq.add(embeddings, labels)
        e = _rank._f32c(embeddings, "embeddings")
        if e.shape[0]:
            a, _ = _cl.assign_clusters(e, self.centroids, eps=self.pq.eps)
            self._set_lists(torch.cat([self.assignments, a]))
        return self

    def _scan(self, q, probes, cap, k, idx_offset, filt):
        pq, dev, L = self.pq, self.pq.device, lib()
        Q, nprobe = q.shape[0], probes.shape[1]
        vals = torch.empty((Q, k), dtype=torch.float32, device=dev)
        idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
        if Q:
            ws = _rank._ws.get(dev, L.mi355_ivfpq_search_workspace_bytes(Q, nprobe, self.nlist, pq.dim, pq.M, cap, k))
            with torch.cuda.device(dev):
                check(L.mi355_ivfpq_search(q.data_ptr(), Q, pq.dim, pq.eps, pq._codebooks.data_ptr(), pq.M,
                                           self.list_codes.data_ptr(), self.rows, self.offsets.data_ptr(), self.order.data_ptr(),
                                           self.nlist, probes.data_ptr(), nprobe, cap, k, int(idx_offset),
                                           None if filt is None else filt[0], vals.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                           ws.numel(), stream_ptr(dev)))
        return vals, idx

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
        self._fresh()
        pq = self.pq
        k, R = _pq._shortlist_length(pq, k, refine, shortlist)
        q, probes = self._probes(queries, nprobe, probes)
        Q, nprobe = q.shape[0], probes.shape[1]
        gl = None if label_filter is None else pq._labels_for(f'label_filter="{label_filter}"')
        filt = _rank._rank_filter(Q, self.rows, q.device, query_labels, gl, label_filter, exclude)
        cap = max(int(self._longest[nprobe]), R)
        vals, idx = self._scan(q, probes.contiguous(), cap, R, idx_offset, filt)
        if refine is None or Q == 0:
            return vals[:, :k], idx[:, :k]
        return _pq._refined_topk(pq, q, vals, idx, k, refine, idx_offset)

    def recall(self, queries: torch.Tensor, k: int, nprobe: int, exact=None, **search_kwargs):
        """(mean, per_query (Q,) float64): the share of the reference's top-k indices that ``search(queries, k, nprobe,
        **search_kwargs)`` returns.  ``exact=None``: the reference is ``pq.search(queries, k)`` - what the lists lose.  A
        ``Gallery`` of the same rows: its exact search - what lists and codes lose together."""
        if exact is not None and (not isinstance(exact, _rank.Gallery) or len(exact) != self.rows):
            raise MI355Error(f"recall needs exact=None or a Gallery of the same {self.rows} rows")
        got = self.search(queries, k, nprobe, **search_kwargs)[1]
        return _rank._recall(got, (self.pq if exact is None else exact).search(queries, k)[1], k)
