"""Product-quantised resident gallery: a row is M bytes, one centroid id of 256 per sub-vector of ``dim / M`` elements - at
D = 1536 and M = 96 a 64th of the fp32 row, so that a million rows are 96 MB and the scan of a query reads bytes, not rows.

* ``PQGallery(dim, device, M, codebooks=None)`` ...... empty gallery; ``codebooks`` (M, 256, dim / M) fp32 if already trained
* ``pq.train(rows, iters=10, seed=0)`` ............... Lloyd per sub-quantiser: ``mi355_pq_encode`` then ``mi355_pq_update``
* ``PQGallery.from_gallery(gallery, M)`` ............. train on an fp32 ``Gallery``, then add its rows and labels
* ``pq.add(embeddings, labels=None)`` ................ normalise and encode (``mi355_pq_encode``)
* ``pq.search(queries, k, refine=None, ...)`` ........ table scan in LDS (``mi355_pq_search``); with ``refine`` a shortlist is
  rescored against the fp32 / fp16 rows of a ``Gallery`` (``mi355_rescore_candidates``) and merged (``merge_topk``)
* ``pq.scores(queries)`` / ``pq.recall(...)`` / ``pq.reconstruct()``

The format is approximate against the fp32 cosine, but its arithmetic is specified bit for bit in include/mi355_retrieval.h: a
score depends on its query, its code row and the codebooks alone, and a NumPy model (tests/pq_ref.py) reproduces every bit of
the codes, the tables, the scores, the top-k and the trained codebooks.  ``pq.ivf(rows, nlist)`` puts IVF lists over the codes
(ivfpq.py).  Growth of the code buffer, labels, recall and the shortlist rules of ``refine=`` come from ``rank._RowStore``, as for
the other galleries.  Codes of a row's offset from its list centroid are ``ResidualIVFPQIndex`` (ivfrpq.py).  Out of scope
(DESIGN §7): an OPQ rotation, a sharded PQ gallery, range search / query expansion over codes, training on fp16 rows.
"""
from __future__ import annotations

import torch

from . import cluster as _cl
from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr

CENTROIDS = 256                     # centroids of every sub-quantiser: a code is one byte
MAX_M, MAX_DSUB = 128, 64
SCAN_CHUNK = 2048                   # rows of one scan workgroup (PQ_CHUNK, csrc/pq.hip)
_is_int = _rank._is_int
_refined_topk = _rank._RowStore._refined_topk       # (store, q, vals, idx, k, refine, idx_offset): the row store's own routine


class PQGallery(_rank._RowStore):
    """Resident product-quantised gallery.  ``codes`` (rows, M) uint8, ``codebooks`` (M, 256, dim / M) fp32.  A search builds
    one table ``T[m][c] = qn_m . codebooks[m][c]`` per query and scores a row as the sum of its M table entries (four
    accumulators, a fixed order); order, ties, NaN queries and pads as ``cosine_topk``.  Equal code rows score equal bits, so
    ties (resolved to the lower row) are common.  A row with a NaN element is encoded like any other (code 0 where the NaN
    reaches): unlike the other galleries it does not rank first."""

    _NOUN = "PQGallery"

    def __init__(self, dim: int, device, M: int, codebooks: torch.Tensor | None = None, capacity: int = 0,
                 eps: float = _rank._EPS):
        super().__init__(dim, device, eps)
        self.M = int(M)
        if self.device.type == "cuda" and self.device.index is None:       # "cuda": the index tensors on it report
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not _is_int(M) or not 4 <= M <= MAX_M or M % 4:
            raise MI355Error(f"a PQGallery needs M a multiple of 4 in [4, {MAX_M}], got {M!r}")
        if self.dim < 1 or self.dim % self.M:
            raise MI355Error(f"a PQGallery needs dim a positive multiple of M={M}, got {dim}")
        self.dsub = self.dim // self.M
        if self.dsub > MAX_DSUB:
            raise MI355Error(f"a PQGallery needs dim / M <= {MAX_DSUB}, got {self.dsub}")
        self._codes = torch.empty((max(int(capacity), 0), self.M), dtype=torch.uint8, device=self.device)
        self._codebooks = None
        self.train_counts = None
        if codebooks is not None:
            cb = _rank._f32c(codebooks, "codebooks")
            if cb.device != self.device or tuple(cb.shape) != (self.M, CENTROIDS, self.dsub):
                raise MI355Error(f"codebooks must be ({self.M}, {CENTROIDS}, {self.dsub}) on {self.device}, got "
                                 f"{tuple(cb.shape)} on {cb.device}")
            self._codebooks = cb

    # ---- the kernels
    def _encode(self, n_rows: torch.Tensor, normalized: bool, out: torch.Tensor) -> None:
        """Codes of the (n, dim) fp32 rows into ``out`` (n, M), a slice of a code buffer."""
        n, L, dev = n_rows.shape[0], lib(), self.device
        need = L.mi355_pq_encode_workspace_bytes(n, self.dim, int(normalized))
        ws = _rank._ws.get(dev, need) if need else None
        with torch.cuda.device(dev):
            check(L.mi355_pq_encode(n_rows.data_ptr(), n, self.dim, self.M, int(normalized), self.eps, self._codebooks.data_ptr(),
                                    out.data_ptr(), n * self.M, ws.data_ptr() if need else None, ws.numel() if need else 0,
                                    stream_ptr(dev)))

    def _update(self, n_rows: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
        """One centroid update from normalised rows and their codes, in place; returns the counts (M, 256) int64."""
        counts = torch.empty((self.M, CENTROIDS), dtype=torch.int64, device=self.device)
        cb = self._codebooks
        with torch.cuda.device(self.device):
            check(lib().mi355_pq_update(n_rows.data_ptr(), n_rows.shape[0], self.dim, self.M, 1, self.eps, codes.data_ptr(),
                                        cb.data_ptr(), cb.data_ptr(), counts.data_ptr(), None, 0, stream_ptr(self.device)))
        return counts

    # ---- training
    def train(self, rows, iters: int = 10, seed: int = 0) -> "PQGallery":
        """Lloyd's algorithm per sub-quantiser on ``rows``, an fp32 device tensor (N, dim) or an fp32 ``Gallery``, N >= 256.
        The start is the sub-vectors of the 256 normalised rows ``cluster.seeded_rows(N, 256, seed)`` picks; an iteration is an
        encode, then an update (the float64 mean of each cell's members in ascending row order; an empty cell keeps its
        centroid).  Deterministic: the same bits for the same rows, seed and ``iters``.  ``train_counts`` (M, 256) int64 holds
        the cell sizes of the last update.  Refused once rows are resident: their codes would name other centroids."""
        if self.rows:
            raise MI355Error(f"train: {self.rows} rows are already resident (their codes belong to the present codebooks)")
        if not _is_int(iters) or iters < 0:
            raise MI355Error(f"train: iters must be a non-negative integer, got {iters!r}")
        if isinstance(rows, _rank.Gallery):
            if rows.dtype != torch.float32:
                raise MI355Error("train: an fp16 Gallery cannot train a PQGallery (training reads fp32 rows)")
            if rows.device != self.device or rows.dim != self.dim:
                raise MI355Error(f"train: the Gallery is ({rows.dim},) on {rows.device}, the PQGallery ({self.dim},) on {self.device}")
            n = rows.data
        else:
            if not torch.is_tensor(rows):
                raise MI355Error(f"train: rows must be a tensor or a Gallery, got {type(rows).__name__}")
            if rows.dtype != torch.float32:
                raise MI355Error(f"train: rows must be fp32, got {rows.dtype}")
            if rows.dim() != 2 or rows.shape[1] != self.dim or rows.device != self.device:
                raise MI355Error(f"train: rows must be (N, {self.dim}) on {self.device}, got {tuple(rows.shape)} on {rows.device}")
            n = rows
        N = int(n.shape[0])
        if N < CENTROIDS:
            raise MI355Error(f"train: {N} rows cannot seed {CENTROIDS} centroids per sub-quantiser")
        if not isinstance(rows, _rank.Gallery):
            n = _rank.l2_normalize_rows(_rank._f32c(n, "rows"), self.eps)
        return self._lloyd(n, iters, seed)

    def _lloyd(self, n: torch.Tensor, iters: int, seed: int) -> "PQGallery":
        """The loop of ``train`` over the (N, dim) fp32 rows ``n`` as they are (``train``: normalised rows; ivfrpq.py: residual
        rows, which are not unit rows and must not be normalised again)."""
        N = int(n.shape[0])
        pick = torch.from_numpy(_cl.seeded_rows(N, CENTROIDS, seed)).to(self.device)
        self._codebooks = n[pick].view(CENTROIDS, self.M, self.dsub).permute(1, 0, 2).contiguous()
        self.train_counts = None
        codes = torch.empty((N, self.M), dtype=torch.uint8, device=self.device)
        for _ in range(int(iters)):
            self._encode(n, True, codes)
            self.train_counts = self._update(n, codes)
        return self

    @classmethod
    def from_gallery(cls, gallery, M: int, iters: int = 10, seed: int = 0) -> "PQGallery":
        """A PQGallery trained on the rows of an fp32 ``Gallery`` and holding them (and its labels)."""
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"from_gallery needs a Gallery, got {type(gallery).__name__}")
        pq = cls(gallery.dim, gallery.device, M, eps=gallery.eps).train(gallery, iters, seed)
        return pq._append(gallery.data, gallery.labels, normalized=True)

    # ---- the resident rows
    _BUFFERS = ("_codes",)

    def _write(self, e: torch.Tensor, r0: int, normalized: bool) -> None:
        self._encode(e, normalized, self._codes[r0: r0 + e.shape[0]])

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None):
        self._trained("add")
        e = self._new_rows(embeddings)
        if e.device != self.device:
            raise MI355Error(f"embeddings are on {e.device} but the gallery lives on {self.device}")
        return self._append(e, labels, normalized=False)

    @property
    def codes(self) -> torch.Tensor:
        """The (rows, M) uint8 codes (a view)."""
        return self._codes[: self.rows]

    @property
    def codebooks(self) -> torch.Tensor | None:
        """The (M, 256, dim / M) fp32 codebooks, or None before ``train``."""
        return self._codebooks

    @property
    def nbytes(self) -> int:
        """Resident footprint in bytes: the codes at the current capacity (M per row) and the codebooks (1024 * dim)."""
        return self._codes.shape[0] * self.M + (0 if self._codebooks is None else self._codebooks.numel() * 4)

    def reconstruct(self) -> torch.Tensor:
        """(rows, dim) fp32: every row as the concatenation of the centroids its codes name."""
        self._trained("reconstruct")
        m = torch.arange(self.M, device=self.device)[None, :]
        return self._codebooks[m, self.codes.long()].reshape(self.rows, self.dim)

    def _trained(self, what: str) -> None:
        if self._codebooks is None:
            raise MI355Error(f"{what}: the PQGallery has no codebooks yet (train() it, or pass codebooks=)")

    def _queries(self, queries: torch.Tensor, what: str) -> torch.Tensor:
        self._trained(what)
        q = _rank._f32c(queries, "queries")
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise MI355Error(f"{what}: queries must be (Q, {self.dim}), got {tuple(q.shape)}")
        if q.device != self.device:
            raise MI355Error(f"{what}: queries are on {q.device} but the gallery lives on {self.device}")
        return q

    # ---- searching
    def scores(self, queries: torch.Tensor) -> torch.Tensor:
        """(Q, rows) fp32: the score of every (query, row) pair, the bits ``search`` ranks by."""
        q = self._queries(queries, "scores")
        Q, G, L = q.shape[0], self.rows, lib()
        out = torch.empty((Q, G), dtype=torch.float32, device=self.device)
        if Q and G:
            ws = _rank._ws.get(self.device, L.mi355_pq_search_workspace_bytes(Q, G, self.dim, self.M, 0))
            with torch.cuda.device(self.device):
                check(L.mi355_pq_scores(q.data_ptr(), Q, self.dim, self.eps, self._codebooks.data_ptr(), self.M,
                                        self._codes.data_ptr(), G, out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(self.device)))
        return out

    def _pq_topk(self, q, k, idx_offset, filt):
        Q, G, L = q.shape[0], self.rows, lib()
        vals = torch.empty((Q, k), dtype=torch.float32, device=self.device)
        idx = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        if Q:
            ws = _rank._ws.get(self.device, L.mi355_pq_search_workspace_bytes(Q, G, self.dim, self.M, k))
            with torch.cuda.device(self.device):
                check(L.mi355_pq_search(q.data_ptr(), Q, self.dim, self.eps, self._codebooks.data_ptr(), self.M,
                                        self._codes.data_ptr(), G, k, int(idx_offset), None if filt is None else filt[0],
                                        vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(self.device)))
        return vals, idx

    def search(self, queries: torch.Tensor, k: int, idx_offset: int = 0, *, query_labels: torch.Tensor | None = None,
               label_filter: str | None = None, exclude: torch.Tensor | None = None, refine=None, shortlist: int | None = None):
        """(values (Q, k) fp32, indices (Q, k) int64), ``1 <= k <= min(1024, rows)``; filters and ``idx_offset`` as in
        ``Gallery.search``.  Without ``refine`` the values are the PQ scores.  With ``refine``, a ``Gallery`` (fp32 or fp16) of
        the same rows on the same device, the PQ search returns ``shortlist`` rows per query (``k <= shortlist <= min(1024,
        rows)``, default ``min(max(10 * k, 100), 1024, rows)``), each is scored again as ``qn . row`` against the gallery's row
        (the bits an ``IVFIndex`` scan gives the pair) and the top-k of those values is returned.  Nothing is read back."""
        self._trained("search")
        k, R = self._shortlist_length(k, refine, shortlist)
        q = self._queries(queries, "search")
        Q = q.shape[0]
        gl = None if label_filter is None else self._labels_for(f'label_filter="{label_filter}"')
        filt = _rank._rank_filter(Q, self.rows, self.device, query_labels, gl, label_filter, exclude)
        vals, idx = self._pq_topk(q, R, idx_offset, filt)
        if refine is None or Q == 0:
            return vals[:, :k], idx[:, :k]
        return self._refined_topk(q, vals, idx, k, refine, idx_offset)

    def recall(self, queries: torch.Tensor, k: int, exact: "_rank.Gallery", **search_kwargs):
        """(mean, per_query (Q,) float64): the share of ``exact.search(queries, k)``'s indices that ``search(queries, k,
        **search_kwargs)`` returns; ``exact`` is a ``Gallery`` of the same rows (pass ``refine=exact`` to measure the refined
        search)."""
        return self._recall_against(exact, queries, k, **search_kwargs)

    def ivf(self, rows, nlist: int, **kw):
        """The ``IVFPQIndex`` over these codes with ``nlist`` lists: ``IVFPQIndex.build(self, rows, nlist, **kw)`` (``iters``,
        ``seed``, ``init``); ``rows`` is the ``Gallery`` or the fp32 tensor the codes were made from."""
        from .ivfpq import IVFPQIndex
        return IVFPQIndex.build(self, rows, nlist, **kw)
