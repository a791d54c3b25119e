"""The inverted-file lists behind ``IVFIndex`` (ivf.py: over a ``Gallery``'s rows) and ``IVFPQIndex`` (ivfpq.py: over a
``PQGallery``'s codes): centroids as the coarse quantiser, the members of every cluster as CSR lists, and the argument rules of
probing them.  A subclass names the store it wraps, builds itself, and scans."""
from __future__ import annotations

import numpy as np
import torch

from . import cluster as _cl
from . import rank as _rank
from ._lib import MI355Error

MAX_K = 1024                        # the largest k of any search, and the most lists a query probes


class _ListIndex:
    """``centroids`` (nlist, D) fp32, ``assignments`` (rows,), ``offsets`` (nlist + 1,) / ``order`` (rows,) int64 (the rows of
    list l are ``order[offsets[l]:offsets[l + 1]]``, ascending) and ``counts`` (nlist,) int64 over the ``rows`` rows that
    ``_store`` held when the lists were made."""

    _NOUN = _STORE_NOUN = _HINT = ""        # the words of the stale message
    _EXTRA = ()                             # the tensors beside the lists that count into nbytes, by attribute name
    _STORE = ""                             # the attribute that holds the gallery the lists are over

    # a subclass also has ``_queries(queries)``: the queries of a search checked against the store, contiguous fp32 (Q, dim)

    @property
    def _store(self):
        return getattr(self, self._STORE)

    def _relist(self) -> None:
        """Called when ``offsets`` and ``order`` have changed, for what a subclass keeps in list order."""

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
