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
returns exactly what ``i8.search`` returns.  The lists, ``probe``, ``stale``, ``add``, ``recall``, the rules for ``nprobe`` /
``probes`` and the search around the scan are ``_lists._ListIndex``, shared with every list index; the query blocks and the scan
call are ``ivf._SlabIndex``, shared with ``IVFIndex``: this class names its two C entries and passes codes and scales.  Out of
scope: a sharded index, k-means over the int8 rows themselves.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import quantized as _q8
from . import rank as _rank
from ._lib import MI355Error
from ._lists import _check_rows, _ListIndex
from .ivf import _SlabIndex

_MAX_SCAN_DIM = 32768               # one query's two planes fill the 64 KB the scan takes


def _check_i8(i8) -> None:
    if not isinstance(i8, _q8.Int8Gallery):
        raise MI355Error(f"an int8 IVF index is built over an Int8Gallery, got {type(i8).__name__}")
    if i8.rows < 1:
        raise MI355Error("an int8 IVF index needs an Int8Gallery with at least one row")
    if i8.dim > _MAX_SCAN_DIM:
        raise MI355Error(f"an int8 IVF index needs dim <= {_MAX_SCAN_DIM}, got {i8.dim}")


class Int8IVFIndex(_SlabIndex):
    """The lists of an ``Int8Gallery``: ``centroids`` (nlist, D) fp32, ``assignments`` (rows,), ``offsets`` (nlist + 1,) /
    ``order`` (rows,) int64 (the rows of list l are ``order[offsets[l]:offsets[l + 1]]``, ascending), ``counts`` (nlist,) int64
    and a reference to ``i8``.  ``stale``: rows were added to ``i8`` behind the index's back (``index.add`` keeps the two
    together)."""

    _STORE, _NOUN, _STORE_NOUN = "i8", "int8 IVF index", "Int8Gallery"
    _HINT = "add rows through index.add, or build the index again"
    _ENTRIES = ("mi355_ivf_scan_i8_workspace_bytes", "mi355_ivf_scan_i8")
    add = _ListIndex._add_to_store

    def __init__(self, i8, centroids: torch.Tensor, assignments: torch.Tensor):
        _check_i8(i8)
        self.i8 = i8
        self._init_lists(self._checked_centroids(centroids), assignments)

    @classmethod
    def build(cls, i8, rows, nlist: int, *, iters: int = 10, seed: int = 0, init: torch.Tensor | None = None) -> "Int8IVFIndex":
        """``spherical_kmeans(rows, nlist, iters=, seed=, init=)``, then the lists of its assignments over ``i8``'s rows.
        ``rows`` is the fp32 / fp16 ``Gallery``, or the (N, D) fp32 tensor, the codes were made from."""
        _check_i8(i8)
        _check_rows(i8, rows)
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

    def _row_args(self):
        return self.i8._codes.data_ptr(), self.i8._scales.data_ptr()

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
        return self._search_lists(queries, k, nprobe, probes, query_labels, label_filter, exclude, idx_offset, refine, shortlist,
                                  block)

    def recall(self, queries: torch.Tensor, k: int, nprobe: int, exact=None, **search_kwargs):
        """(mean, per_query (Q,) float64): the share of the reference's top-k indices that ``search(queries, k, nprobe,
        **search_kwargs)`` returns.  ``exact=None``: the reference is ``i8.search(queries, k)`` - what the lists lose.  A
        ``Gallery`` of the same rows: its exact search - what lists and codes lose together."""
        return self._recall_lists(queries, k, nprobe, exact, **search_kwargs)
