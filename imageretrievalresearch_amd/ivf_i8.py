"""IVF search over the codes of an ``Int8Gallery``: inverted-file lists over the project's smallest real-row format.  The
centroids of a spherical k-means of the rows the codes were made from are the coarse quantiser; a query reads the int8 rows of
the ``nprobe`` lists nearest to it only, a quarter of the bytes an ``IVFIndex`` over fp32 rows reads for the same lists.

* ``Int8IVFIndex(i8, centroids, assignments)`` ....... the lists of given assignments over ``i8``'s rows
* ``Int8IVFIndex.build(i8, rows, nlist)`` ............ ``spherical_kmeans`` of ``rows`` (the ``Gallery`` or the fp32 tensor the
  codes were made from), then the constructor (``Int8Gallery.ivf`` caches it)
* ``Int8IVFIndex.from_gallery(gallery, nlist)`` ...... ``gallery.quantized()`` under the lists of ``gallery.ivf(nlist)``
* ``index.probe(queries, nprobe)`` ................... the nearest lists: the fp32 top-k of the queries against the centroids
* ``index.search(queries, k, nprobe, refine=None)`` .. scan of the probed lists (``mi355_ivf_scan_i8``), ``merge_topk``,
  ``clear_pads``; with ``refine`` a shortlist is rescored against the fp32 / fp16 rows of a ``Gallery``
* ``index.recall(queries, k, nprobe, exact=None)`` ... against ``i8.search`` (what the lists lose) or a ``Gallery``
* ``index.add(embeddings, labels=None)`` ............. ``i8.add``, the new rows to their nearest lists, the lists again

The rows are scanned where they lie in the gallery, through the lists' ``order``: the index holds no copy of the codes.  A score
is the int8 score of the gallery's own row, bit for bit (the integer sums are exact), so a search that probes every list
returns exactly what ``i8.search`` returns.  The lists, ``probe``, ``stale`` and the rules for ``nprobe`` / ``probes`` are
``_lists._ListIndex``, shared with ``IVFIndex`` and ``IVFPQIndex``.  Out of scope: a sharded index, k-means over
the int8 rows themselves.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import ivf as _ivf
from . import pq as _pq
from . import quantized as _q8
from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr
from ._lists import _ListIndex
from .ivfpq import IVFPQIndex

_MAX_SCAN_DIM = 32768               # one query's two planes fill the 64 KB the scan takes


def _check_i8(i8) -> None:
    if not isinstance(i8, _q8.Int8Gallery):
        raise MI355Error(f"an int8 IVF index is built over an Int8Gallery, got {type(i8).__name__}")
    if i8.rows < 1:
        raise MI355Error("an int8 IVF index needs an Int8Gallery with at least one row")
    if i8.dim > _MAX_SCAN_DIM:
        raise MI355Error(f"an int8 IVF index needs dim <= {_MAX_SCAN_DIM}, got {i8.dim}")


class Int8IVFIndex(_ListIndex):
    """The lists of an ``Int8Gallery``: ``centroids`` (nlist, D) fp32, ``assignments`` (rows,), ``offsets`` (nlist + 1,) /
    ``order`` (rows,) int64 (the rows of list l are ``order[offsets[l]:offsets[l + 1]]``, ascending), ``counts`` (nlist,) int64
    and a reference to ``i8``.  ``stale``: rows were added to ``i8`` behind the index's back (``index.add`` keeps the two
    together)."""

    _STORE, _NOUN, _STORE_NOUN = "i8", "int8 IVF index", "Int8Gallery"
    _HINT = "add rows through index.add, or build the index again"

    def __init__(self, i8, centroids: torch.Tensor, assignments: torch.Tensor):
        _check_i8(i8)
        self.i8 = i8
        if not torch.is_tensor(centroids):
            raise MI355Error(f"centroids must be a tensor, got {type(centroids).__name__}")
        c = centroids
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != i8.dim or c.device != i8.device:
            raise MI355Error(f"centroids must be (nlist, {i8.dim}) on {i8.device}, got {tuple(c.shape)} on {c.device}")
        self._init_lists(_rank._f32c(c, "centroids"), assignments)

    @classmethod
    def build(cls, i8, rows, nlist: int, *, iters: int = 10, seed: int = 0, init: torch.Tensor | None = None) -> "Int8IVFIndex":
        """``spherical_kmeans(rows, nlist, iters=, seed=, init=)``, then the lists of its assignments over ``i8``'s rows.
        ``rows`` is the fp32 / fp16 ``Gallery``, or the (N, D) fp32 tensor, the codes were made from."""
        _check_i8(i8)
        IVFPQIndex._check_rows(i8, rows)
        r = _cl.spherical_kmeans(rows, nlist, iters=iters, seed=seed, init=init, eps=i8.eps)
        return cls(i8, r.centroids, r.assignments)

    @classmethod
    def from_gallery(cls, gallery, nlist: int, **kmeans_kw) -> "Int8IVFIndex":
        """``gallery.quantized()`` under the centroids and assignments of ``gallery.ivf(nlist, **kmeans_kw)``: the two indexes
        can be compared list for list."""
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"from_gallery needs a Gallery, got {type(gallery).__name__}")
        i8 = gallery.quantized()
        fp = gallery.ivf(nlist, **kmeans_kw)
        return cls(i8, fp.centroids, fp.assignments)

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None) -> "Int8IVFIndex":
        """``i8.add(embeddings, labels)``, then ``assign_clusters`` of the new fp32 rows against the unchanged centroids, then
        the lists again."""
        self._fresh()
        self.i8.add(embeddings, labels)
        e = _rank._f32c(embeddings, "embeddings")
        if e.shape[0]:
            a, _ = _cl.assign_clusters(e, self.centroids, eps=self.i8.eps)
            self._set_lists(torch.cat([self.assignments, a]))
        return self

    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        q = _rank._f32c(queries, "queries")
        _rank._check_qg(q, self.i8._resident())
        return q

    _block = _ivf.IVFIndex._block

    def _scan(self, q, probes, cap, idx_offset, filt):
        """The candidate slab (values (n, cap) fp32, indices (n, cap) int64) of the queries ``q`` (n, D) probing ``probes``."""
        g = self.i8
        n, nprobe, dev = q.shape[0], probes.shape[1], q.device
        cand_val = torch.empty((n, cap), dtype=torch.float32, device=dev)
        cand_idx = torch.empty((n, cap), dtype=torch.int64, device=dev)
        L = lib()
        ws = _rank._ws.get(dev, L.mi355_ivf_scan_i8_workspace_bytes(n, nprobe, self.nlist, g.dim, cap))
        with torch.cuda.device(dev):
            check(L.mi355_ivf_scan_i8(q.data_ptr(), n, g.dim, g.eps, g._codes.data_ptr(), g._scales.data_ptr(), g._ld, g.rows,
                                      self.offsets.data_ptr(), self.order.data_ptr(), self.nlist, probes.data_ptr(), nprobe, cap,
                                      int(idx_offset), None if filt is None else filt[0], cand_val.data_ptr(),
                                      cand_idx.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(dev)))
        return cand_val, cand_idx

    def search(self, queries: torch.Tensor, k: int, nprobe: int | None = None, *, probes: torch.Tensor | None = None,
               query_labels: torch.Tensor | None = None, label_filter: str | None = None, exclude: torch.Tensor | None = None,
               idx_offset: int = 0, block: int | None = None, refine=None, shortlist: int | None = None):
        """(values (Q, k) fp32, indices (Q, k) int64): the top-k of the rows of every query's probed lists, scored and ordered
        as ``Int8Gallery.search`` scores and orders them (descending, NaN first, ties to the lower gallery row).  Exactly one
        of ``nprobe`` (the lists of ``probe(queries, nprobe)``) and ``probes`` ((Q, n) int64 list ids, distinct within a row)
        is given.  A score depends on its query and its row only: not on the other queries, ``nprobe`` or ``block``; probing
        every list returns ``i8.search``'s result bit for bit.  Filters and ``idx_offset`` as in ``Gallery.search``; with fewer
        than k eligible probed rows the remaining slots are (-inf, -1).  ``1 <= k <= min(1024, rows)``.  ``refine`` and
        ``shortlist`` as in ``PQGallery.search`` (the shortlist comes from the probed lists).  The queries go through
        ``block`` at a time (default: what keeps the candidate slab under 256 MB); the result does not depend on it."""
        self._fresh()
        g = self.i8
        k, R = _pq._shortlist_length(g, k, refine, shortlist)
        q, probes = self._probes(queries, nprobe, probes)
        Q, nprobe = q.shape[0], probes.shape[1]
        gl = None if label_filter is None else g._labels_for(f'label_filter="{label_filter}"')
        filtered = _rank._rank_filter(Q, g.rows, q.device, query_labels, gl, label_filter, exclude) is not None
        cap = max(int(self._longest[nprobe]), R)
        blk = self._block(Q, nprobe, cap, block)
        vals = torch.empty((Q, R), dtype=torch.float32, device=q.device)
        idx = torch.empty((Q, R), dtype=torch.int64, device=q.device)
        for q0 in range(0, Q, blk):
            q1 = min(Q, q0 + blk)
            filt = None
            if filtered:
                filt = _rank._rank_filter(q1 - q0, g.rows, q.device, None if query_labels is None else query_labels[q0:q1], gl,
                                          label_filter, None if exclude is None else exclude[q0:q1])
            cand_val, cand_idx = self._scan(q[q0:q1], probes[q0:q1].contiguous(), cap, idx_offset, filt)
            v, i = _rank.merge_topk(cand_val, cand_idx, R)
            _rank.clear_pads(v, i, int(idx_offset), int(idx_offset) + g.rows)
            vals[q0:q1], idx[q0:q1] = v, i
        if refine is None or Q == 0:
            return vals, idx
        return _pq._refined_topk(g, q, vals, idx, k, refine, idx_offset)

    def recall(self, queries: torch.Tensor, k: int, nprobe: int, exact=None, **search_kwargs):
        """(mean, per_query (Q,) float64): the share of the reference's top-k indices that ``search(queries, k, nprobe,
        **search_kwargs)`` returns.  ``exact=None``: the reference is ``i8.search(queries, k)`` - what the lists lose.  A
        ``Gallery`` of the same rows: its exact search - what lists and codes lose together."""
        if exact is not None and (not isinstance(exact, _rank.Gallery) or len(exact) != self.rows):
            raise MI355Error(f"recall needs exact=None or a Gallery of the same {self.rows} rows")
        got = self.search(queries, k, nprobe, **search_kwargs)[1]
        return _rank._recall(got, (self.i8 if exact is None else exact).search(queries, k)[1], k)
