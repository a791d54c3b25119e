"""The inverted-file lists behind ``IVFIndex`` (ivf.py: over a ``Gallery``'s rows), ``Int8IVFIndex`` (ivf_i8.py: an
``Int8Gallery``'s), ``IVFPQIndex`` (ivfpq.py: a ``PQGallery``'s codes) and ``ResidualIVFPQIndex`` (ivfrpq.py): centroids as the
coarse quantiser, the members of every cluster as CSR lists, the argument rules of probing them, and the one search every index
runs (``_search_lists``: the checks, the probes, the filter, the scan of a subclass, the refine tail).  A subclass names the
store it wraps, builds itself, and says in ``_top_of_lists`` how the probed lists are scanned."""
from __future__ import annotations

import numpy as np
import torch

from . import cluster as _cl
from . import rank as _rank
from ._lib import MI355Error

MAX_K = _rank._MAX_K                # the largest k of any search, and the most lists a query probes


def _check_rows(store, rows) -> None:
    """``rows``: what ``store``'s codes were made from - a Gallery (fp32 or fp16) or a (N, D) fp32 tensor, same device and dim,
    N == len(store).  ``store``: a ``PQGallery`` or an ``Int8Gallery``."""
    if isinstance(rows, _rank.Gallery):
        n, dim, dev = len(rows), rows.dim, rows.device
    elif torch.is_tensor(rows):
        if rows.dtype != torch.float32:
            raise MI355Error(f"rows must be fp32, got {rows.dtype} (an fp16 Gallery is accepted; fp16 tensors are not)")
        if rows.dim() != 2:
            raise MI355Error(f"rows must be (N, {store.dim}), got {tuple(rows.shape)}")
        n, dim, dev = int(rows.shape[0]), int(rows.shape[1]), rows.device
    else:
        raise MI355Error(f"rows must be a Gallery or a tensor, got {type(rows).__name__}")
    if dev != store.device:
        raise MI355Error(f"rows are on {dev} but the {store._NOUN} lives on {store.device}")
    if dim != store.dim:
        raise MI355Error(f"rows have dim {dim}, the {store._NOUN} {store.dim}")
    if n != store.rows:
        raise MI355Error(f"rows holds {n} rows, the {store._NOUN} {store.rows}: the lists are made of the rows the codes were made from")


class _ListIndex:
    """``centroids`` (nlist, D) fp32, ``assignments`` (rows,), ``offsets`` (nlist + 1,) / ``order`` (rows,) int64 (the rows of
    list l are ``order[offsets[l]:offsets[l + 1]]``, ascending) and ``counts`` (nlist,) int64 over the ``rows`` rows that
    ``_store`` held when the lists were made."""

    _NOUN = _STORE_NOUN = _HINT = ""        # the words of the stale message
    _EXTRA = ()                             # the tensors beside the lists that count into nbytes, by attribute name
    _STORE = ""                             # the attribute that holds the gallery the lists are over

    # a subclass also has ``_queries(queries)``: the queries of a search checked against the store, contiguous fp32 (Q, dim),
    # and ``_top_of_lists(q, probes, cap, R, idx_offset, filt, block)``: (values, indices) (Q, R), the top-R of the probed lists

    @property
    def _store(self):
        return getattr(self, self._STORE)

    def _relist(self) -> None:
        """Called when ``offsets`` and ``order`` have changed, for what a subclass keeps in list order."""

    def _checked_centroids(self, c) -> torch.Tensor:
        """A caller's ``centroids`` as contiguous fp32 (nlist, dim) on the store's device (``IVFIndex``: ``_cl._centroids_of``)."""
        store = self._store
        if not torch.is_tensor(c):
            raise MI355Error(f"centroids must be a tensor, got {type(c).__name__}")
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != store.dim or c.device != store.device:
            raise MI355Error(f"centroids must be (nlist, {store.dim}) on {store.device}, got {tuple(c.shape)} on {c.device}")
        return _rank._f32c(c, "centroids")

    def _init_lists(self, centroids: torch.Tensor, assignments: torch.Tensor) -> None:
        self.centroids = centroids
        self.nlist = int(centroids.shape[0])
        if self.nlist >= 1 << 24:
            raise MI355Error(f"nlist={self.nlist} must be below 2^24")
        self._set_lists(_rank._int64_on(assignments, "assignments", self._store.rows, self._store.device))

    def _set_lists(self, assignments: torch.Tensor) -> None:
        self.assignments = assignments
        self.offsets, self.order = _cl.cluster_members(assignments, self.nlist)
        self.counts = self.offsets[1:] - self.offsets[:-1]
        self._relist()
        host = self.counts.cpu().numpy()                                    # the one read of the lists' lengths
        self._longest = np.concatenate([[0], np.cumsum(np.sort(host)[::-1])])   # [n] = the rows of the n longest lists
        self.rows = int(assignments.shape[0])

    @property
    def nbytes(self) -> int:
        """The index's size in bytes: centroids, assignments, offsets, order and counts, and what the index keeps in list
        order; the rows or codes themselves belong to the gallery."""
        own = (self.centroids, self.assignments, self.offsets, self.order, self.counts) + tuple(getattr(self, n) for n in self._EXTRA)
        return sum(t.numel() * t.element_size() for t in own)

    @property
    def stale(self) -> bool:
        """Rows were added to the gallery since the lists were made."""
        return self.rows != self._store.rows

    def _fresh(self) -> None:
        if self.stale:
            raise MI355Error(f"the {self._NOUN} is stale: it lists {self.rows} rows but the {self._STORE_NOUN} holds "
                             f"{self._store.rows} ({self._HINT})")

    def _check_nprobe(self, nprobe) -> int:
        top = min(self.nlist, MAX_K)
        if not _rank._is_int(nprobe) or not 1 <= nprobe <= top:
            raise MI355Error(f"nprobe={nprobe!r} outside [1, {top}] (min(nlist, {MAX_K}))")
        return int(nprobe)

    def probe(self, queries: torch.Tensor, nprobe: int) -> torch.Tensor:
        """(Q, nprobe) int64: the lists nearest to every query, nearest first - exactly the indices of
        ``cosine_topk(queries, centroids, nprobe)``.  ``1 <= nprobe <= min(nlist, 1024)``."""
        nprobe = self._check_nprobe(nprobe)
        return _rank.cosine_topk(queries, self.centroids, nprobe, self._store.eps)[1]

    def _probes(self, queries: torch.Tensor, nprobe, probes):
        """(q, probes): the checked queries and the (Q, nprobe) int64 lists each of them probes - ``probe(q, nprobe)``, or the
        caller's ``probes``; exactly one of the two is given.  Counts are checked before anything that needs the GPU."""
        if (nprobe is None) == (probes is None):
            raise MI355Error("give exactly one of nprobe and probes")
        if probes is not None and (not torch.is_tensor(probes) or probes.dim() != 2):
            raise MI355Error("probes must be a (Q, nprobe) tensor")
        nprobe = self._check_nprobe(nprobe if probes is None else int(probes.shape[1]))
        q = self._queries(queries)
        Q = q.shape[0]
        if probes is None:
            return q, (self.probe(q, nprobe) if Q else torch.empty((0, nprobe), dtype=torch.int64, device=q.device))
        if probes.shape[0] != Q:
            raise MI355Error(f"probes must be a (Q={Q}, nprobe) tensor, got {tuple(probes.shape)}")
        return q, _rank._int64_on(probes.reshape(-1), "probes", Q * nprobe, q.device).view(Q, nprobe)

    def _add_to_store(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None):
        """The store's ``add(embeddings, labels)``, then ``assign_clusters`` of the new fp32 rows against the unchanged
        centroids, then the lists (and what the index keeps in list order) again.  Returns the index.  It is the ``add`` of
        the indexes whose store grows through them (``IVFPQIndex``, ``Int8IVFIndex``)."""
        self._fresh()
        self._store.add(embeddings, labels)
        e = _rank._f32c(embeddings, "embeddings")
        if e.shape[0]:
            a, _ = _cl.assign_clusters(e, self.centroids, eps=self._store.eps)
            self._set_lists(torch.cat([self.assignments, a]))
        return self

    def _search_lists(self, queries, k, nprobe, probes, query_labels, label_filter, exclude, idx_offset, refine=None,
                      shortlist=None, block=None):
        """The ``search`` of every list index: the checks in their one order, the probes, the filter of the whole batch, the
        subclass's ``_top_of_lists``, and with ``refine`` the rescoring of the shortlist."""
        self._fresh()
        store = self._store
        k, R = store._shortlist_length(k, refine, shortlist)
        q, probes = self._probes(queries, nprobe, probes)
        Q, nprobe = q.shape[0], probes.shape[1]
        gl = None if label_filter is None else store._labels_for(f'label_filter="{label_filter}"')
        filt = _rank._rank_filter(Q, store.rows, q.device, query_labels, gl, label_filter, exclude)
        cap = max(int(self._longest[nprobe]), R)
        vals, idx = self._top_of_lists(q, probes, cap, R, idx_offset, filt, block)
        if refine is not None and Q:
            return store._refined_topk(q, vals, idx, k, refine, idx_offset)
        return (vals, idx) if R == k else (vals[:, :k], idx[:, :k])         # R > k: a shortlist of no query

    def _recall_lists(self, queries, k, nprobe, exact, needs_exact: bool = False, **search_kwargs):
        """(mean, per_query): the share of the reference's top-k that ``search(queries, k, nprobe, **search_kwargs)`` returns.
        The reference is the search of ``exact``, a ``Gallery`` of the same rows, or of the store itself when ``exact`` is None."""
        if (exact is not None or needs_exact) and (not isinstance(exact, _rank.Gallery) or len(exact) != self.rows):
            raise MI355Error(f"recall needs {'exact,' if needs_exact else 'exact=None or'} a Gallery of the same {self.rows} rows")
        got = self.search(queries, k, nprobe, **search_kwargs)[1]
        return _rank._recall(got, (self._store if exact is None else exact).search(queries, k)[1], k)
