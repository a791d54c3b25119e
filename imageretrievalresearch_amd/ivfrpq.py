"""Residual IVF-PQ: an ``IVFPQIndex`` whose codes describe a row's offset from the centroid of its list, ``rn - centroids[l]``,
not the whole unit row.  The k-means lists then pay for accuracy as well as for time: the codebooks spend their 256 centroids per
sub-quantiser on what is left of a row once its cluster centre is taken away.

* ``ResidualIVFPQIndex(centroids, codebooks)`` ........... empty index over unit centroids (nlist, D) and residual codebooks
* ``ResidualIVFPQIndex.build(rows, M, nlist)`` ........... ``spherical_kmeans``, residuals of the training rows, Lloyd on them
  (``PQGallery.train``'s loop), then every row added (``from_gallery`` is the same call)
* ``index.add(embeddings, labels=None, assignments=None)`` normalise, ``assign_clusters`` unless given, residuals
  (``mi355_ivfpq_residuals``), encode (``mi355_pq_encode``), the lists and ``list_codes`` again
* ``index.search(queries, k, nprobe, refine=None, ...)`` .. ``IVFPQIndex.search`` itself; its scan call names
  ``mi355_ivfpq_residual_search`` and takes the centroids as well
* ``index.coarse(queries, probes)`` ...................... (Q, nprobe) fp32: the query . centroid terms of the scores
* ``index.probe`` / ``index.recall(queries, k, nprobe, exact)`` / ``index.reconstruct()``
* ``index.codes`` / ``list_codes`` / ``codebooks`` / ``labels`` / ``nbytes``

The score of (query, row) is ``coarse(q, list of the row) + the PQ score of the row's residual code``, specified bit for bit in
include/mi355_retrieval.h; tests/ivfrpq_ref.py is the NumPy model.  With inner products there is still one table per query
(``q . residual centroid`` does not depend on the list) and one scalar per (query, probed list).  The codes live in a
``PQGallery`` of the residual codebooks (``index.pq``: growth and labels are ``rank._RowStore``'s); the lists, the search
around the scan and ``recall`` are ``_lists._ListIndex``, the scan call is ``IVFPQIndex._scan``.  Out of scope: an
OPQ rotation, a sharded index, training on fp16 rows.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import pq as _pq
from . import rank as _rank
from ._lib import DTYPE_F32, MI355Error, check, lib, stream_ptr
from .ivfpq import IVFPQIndex

ENCODE_BLOCK = 16384                # rows whose residuals exist at one time while rows are encoded
_RESIDUALS_WS = 512                 # MI355_IVFPQ_RESIDUALS_WORKSPACE


def _residuals(rows: torch.Tensor, normalized: bool, assignments: torch.Tensor, centroids: torch.Tensor, eps: float,
               out: torch.Tensor) -> torch.Tensor:
    """``out`` (n, D) = normalised ``rows`` (n, D) minus ``centroids[assignments]``; an assignment outside the lists raises."""
    n, dev = rows.shape[0], rows.device
    if n:
        ws = _rank._ws.get(dev, _RESIDUALS_WS)
        with torch.cuda.device(dev):
            check(lib().mi355_ivfpq_residuals(rows.data_ptr(), n, rows.shape[1], int(normalized), eps, assignments.data_ptr(),
                                              centroids.data_ptr(), centroids.shape[0], out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              stream_ptr(dev)))
    return out


class _ResidualCodes(_pq.PQGallery):
    """The row store of the index: a ``PQGallery`` of the residual codebooks whose rows are written as the codes of their
    residuals, ``ENCODE_BLOCK`` rows at a time."""

    def _write(self, e: torch.Tensor, r0: int, normalized: bool, assignments: torch.Tensor, centroids: torch.Tensor) -> None:
        n = e.shape[0]
        res = torch.empty((min(n, ENCODE_BLOCK), self.dim), dtype=torch.float32, device=self.device)
        for b in range(0, n, ENCODE_BLOCK):
            m = min(ENCODE_BLOCK, n - b)
            _residuals(e[b: b + m], normalized, assignments[b: b + m], centroids, self.eps, res[:m])
            self._encode(res[:m], True, self._codes[r0 + b: r0 + b + m])


class ResidualIVFPQIndex(IVFPQIndex):
    """``centroids`` (nlist, D) fp32 unit rows, ``codebooks`` (M, 256, D / M) fp32 of residual sub-vectors, ``codes`` (rows, M)
    uint8, ``assignments`` / ``offsets`` / ``order`` / ``counts`` as in ``IVFPQIndex``, ``list_codes`` (rows, M) the codes in list
    order.  ``pq`` is the store of the codes; searching it directly is meaningless (its codes are residuals)."""

    _NOUN, _STORE_NOUN = "residual IVF-PQ index", "code store"
    _HINT = "add rows through index.add"
    _ENTRIES = ("mi355_ivfpq_residual_search_workspace_bytes", "mi355_ivfpq_residual_search")

    def __init__(self, centroids: torch.Tensor, codebooks: torch.Tensor, eps: float = _rank._EPS):
        if not torch.is_tensor(centroids) or centroids.dim() != 2 or centroids.shape[0] < 1:
            raise MI355Error("centroids must be a (nlist, D) tensor")
        if not torch.is_tensor(codebooks) or codebooks.dim() != 3:
            raise MI355Error("codebooks must be a (M, 256, D / M) tensor")
        c = _rank._f32c(centroids, "centroids")
        if c.shape[0] >= 1 << 24:
            raise MI355Error(f"nlist={c.shape[0]} must be below 2^24")
        self.pq = _ResidualCodes(int(c.shape[1]), c.device, int(codebooks.shape[0]), codebooks=codebooks, eps=eps)
        self.centroids, self.nlist, dev = c, int(c.shape[0]), c.device
        # the lists of no rows
        self.assignments = torch.empty(0, dtype=torch.int64, device=dev)
        self.order = torch.empty(0, dtype=torch.int64, device=dev)
        self.offsets = torch.zeros(self.nlist + 1, dtype=torch.int64, device=dev)
        self.counts = self.offsets[1:] - self.offsets[:-1]
        self._longest = [0] * (self.nlist + 1)
        self.rows = 0
        self.list_codes = self.pq.codes

    # ---- building
    @staticmethod
    def _source(rows):
        """(n, normalized, eps, labels): the (N, D) fp32 rows a build reads, whether they are unit rows already, and what a
        ``Gallery`` brings along."""
        if isinstance(rows, _rank.Gallery):
            if rows.dtype != torch.float32:
                raise MI355Error("build: an fp16 Gallery cannot train residual codebooks (training reads fp32 rows)")
            return None, True, rows.eps, rows.labels
        if not torch.is_tensor(rows):
            raise MI355Error(f"build: rows must be a Gallery or a tensor, got {type(rows).__name__}")
        if rows.dtype != torch.float32:
            raise MI355Error(f"build: rows must be fp32, got {rows.dtype}")
        if rows.dim() != 2:
            raise MI355Error(f"build: rows must be (N, D), got {tuple(rows.shape)}")
        return rows, False, _rank._EPS, None

    @classmethod
    def build(cls, rows, M: int, nlist: int, *, labels: torch.Tensor | None = None, iters: int = 10, pq_iters: int = 10,
              seed: int = 0, init: torch.Tensor | None = None, train_rows: int | None = None) -> "ResidualIVFPQIndex":
        """``spherical_kmeans(rows, nlist, iters=, seed=, init=)`` gives the centroids and the lists; the residuals of the
        training rows - all of them, or the ``train_rows`` rows ``cluster.seeded_rows(N, train_rows, seed)`` picks, in that
        order - train the codebooks (``pq_iters`` Lloyd steps from the residuals of the rows ``seeded_rows(n_train, 256, seed)``
        picks); then every row is encoded.  ``rows``: an fp32 ``Gallery`` (its labels come along unless ``labels`` is given) or a
        (N, D) fp32 device tensor, N >= 256."""
        n, normalized, eps, own_labels = cls._source(rows)
        N, dim, dev = (len(rows), rows.dim, rows.device) if n is None else (int(n.shape[0]), int(n.shape[1]), n.device)
        store = _pq.PQGallery(dim, dev, M, eps=eps)                    # (the rules for M and dim)
        if not _rank._is_int(pq_iters) or pq_iters < 0:
            raise MI355Error(f"build: pq_iters must be a non-negative integer, got {pq_iters!r}")
        n_train = N if train_rows is None else train_rows
        if not _rank._is_int(n_train) or not _pq.CENTROIDS <= n_train <= N:
            raise MI355Error(f"build: {n_train!r} training rows of {N}: {_pq.CENTROIDS} centroids per sub-quantiser need "
                             f"train_rows in [{_pq.CENTROIDS}, N]")
        r = _cl.spherical_kmeans(rows, nlist, iters=iters, seed=seed, init=init, eps=eps)
        n = rows.data if n is None else _rank._f32c(n, "rows")
        if train_rows is None:
            t, a = n, r.assignments
        else:
            pick = torch.from_numpy(_cl.seeded_rows(N, n_train, seed)).to(dev)
            t, a = n[pick], r.assignments[pick]
        res = _residuals(t, normalized, a, r.centroids, eps, torch.empty((n_train, dim), dtype=torch.float32, device=dev))
        store._lloyd(res, pq_iters, seed)
        del res
        index = cls(r.centroids, store.codebooks, eps=eps)
        return index._add(n, own_labels if labels is None else labels, r.assignments, normalized)

    @classmethod
    def from_gallery(cls, gallery, M: int, nlist: int, **kw) -> "ResidualIVFPQIndex":
        """``build(gallery, M, nlist, **kw)`` over an fp32 ``Gallery``."""
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"from_gallery needs a Gallery, got {type(gallery).__name__}")
        return cls.build(gallery, M, nlist, **kw)

    def _add(self, e: torch.Tensor, labels, assignments: torch.Tensor, normalized: bool) -> "ResidualIVFPQIndex":
        self.pq._append(e, labels, normalized=normalized, assignments=assignments, centroids=self.centroids)
        if e.shape[0]:
            self._set_lists(torch.cat([self.assignments, assignments]))
        return self

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None,
            assignments: torch.Tensor | None = None) -> "ResidualIVFPQIndex":
        """The rows behind those held: normalised, put into the list ``assignments`` (n,) names (default: the nearest centroid,
        ``assign_clusters``), coded as their residuals; then the lists and ``list_codes`` again."""
        self._fresh()
        pq = self.pq
        if not torch.is_tensor(embeddings) or embeddings.dim() != 2 or embeddings.shape[1] != pq.dim:
            raise MI355Error(f"embeddings must be a (n, {pq.dim}) tensor")
        n = int(embeddings.shape[0])
        if assignments is not None and (not torch.is_tensor(assignments) or assignments.dim() != 1 or assignments.shape[0] != n):
            raise MI355Error(f"assignments must have shape ({n},), one list per new row")
        if embeddings.device != pq.device:
            raise MI355Error(f"embeddings are on {embeddings.device} but the index lives on {pq.device}")
        e = pq._new_rows(embeddings)
        if assignments is None:
            a = _cl.assign_clusters(e, self.centroids, eps=pq.eps)[0] if n else self.assignments[:0]
        else:
            a = _rank._int64_on(assignments, "assignments", n, pq.device)
        return self._add(e, labels, a, False)

    # ---- searching
    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        pq = self.pq
        if not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != pq.dim:
            raise MI355Error(f"queries must be (Q, {pq.dim})")
        if queries.device != pq.device:
            raise MI355Error(f"queries are on {queries.device} but the index lives on {pq.device}")
        return pq._queries(queries, "search")

    def _scan_args(self):
        return (self.centroids.data_ptr(),)

    def coarse(self, queries: torch.Tensor, probes: torch.Tensor) -> torch.Tensor:
        """(Q, nprobe) fp32: ``qn . centroids[probes[q, j]]``, the term a search adds to the PQ score of every row of that list
        (``mi355_rescore_candidates`` over the centroids: the same bits); -inf for a list id outside the lists."""
        q, probes = self._probes(queries, None, probes)
        Q, nprobe, L, dev = q.shape[0], probes.shape[1], lib(), self.pq.device
        out = torch.empty((Q, nprobe), dtype=torch.float32, device=dev)
        if Q:
            probes = probes.contiguous()
            ws = _rank._ws.get(dev, L.mi355_rescore_candidates_workspace_bytes(Q, self.pq.dim))
            with torch.cuda.device(dev):
                check(L.mi355_rescore_candidates(q.data_ptr(), Q, self.pq.dim, self.pq.eps, self.centroids.data_ptr(), DTYPE_F32,
                                                 self.pq.dim, self.nlist, probes.data_ptr(), nprobe, 0, out.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), stream_ptr(dev)))
        return out

    def recall(self, queries: torch.Tensor, k: int, nprobe: int, exact, **search_kwargs):
        """(mean, per_query (Q,) float64): the share of ``exact.search(queries, k)``'s indices that ``search(queries, k,
        nprobe, **search_kwargs)`` returns; ``exact`` is a ``Gallery`` of the same rows."""
        return self._recall_lists(queries, k, nprobe, exact, True, **search_kwargs)

    def reconstruct(self) -> torch.Tensor:
        """(rows, dim) fp32: ``centroids[assignments]`` plus the centroids each row's residual codes name."""
        self._fresh()
        return self.centroids[self.assignments] + self.pq.reconstruct()

    # ---- what the index holds
    @property
    def codes(self) -> torch.Tensor:
        """The (rows, M) uint8 residual codes in gallery order (a view)."""
        return self.pq.codes

    @property
    def codebooks(self) -> torch.Tensor:
        """The (M, 256, dim / M) fp32 residual codebooks."""
        return self.pq.codebooks

    @property
    def labels(self) -> torch.Tensor | None:
        return self.pq.labels

    @property
    def nbytes(self) -> int:
        """Resident bytes: the codes at their capacity and the codebooks, the lists, the centroids and ``list_codes``."""
        return super().nbytes + self.pq.nbytes
