"""Binary (sign-bit) resident gallery: a row is ``dim`` bits, bit j set iff element j of the normalised row reaches a trained
centre - at D = 1536 a row is 192 bytes, twice the PQ row at M = 96 and an eighth of the int8 row.  The score of a pair is the
cosine of the two +-1 vectors, ``(dim - 2 h) / dim`` with ``h`` the Hamming distance: one xor and one accumulating popcount per
32 dimensions, no table and no gather, and a gallery row held in registers is reused by a whole block of queries - the batched
exhaustive first stage that the PQ table scan (one query per workgroup) is not.

* ``BinaryGallery(dim, device, center=None)`` ........ empty gallery; ``center`` (dim,) fp32 if already known (None: zeros)
* ``bg.train(rows)`` ................................ ``center`` = the column mean of the normalised rows (``embedding_moments``)
* ``BinaryGallery.from_gallery(gallery)`` ........... train on an fp32 ``Gallery``, then add its rows and labels
* ``bg.add(embeddings, labels=None)`` ............... normalise and encode (``mi355_binary_encode``)
* ``bg.search(queries, k, refine=None, ...)`` ....... popcount scan (``mi355_binary_search``); with ``refine`` a shortlist is
  rescored against the fp32 / fp16 rows of a ``Gallery`` (``mi355_rescore_candidates``) and merged (``merge_topk``)
* ``bg.distances(queries)`` / ``bg.recall(...)``
* ``asymmetric=True`` (``search``, ``distances``, ``recall``): the gallery stays bits, the query keeps 8 bits per element - int8
  codes ``u`` of ``n - center`` - and a row's distance is the Hamming distance weighted by ``|u|``
  (``mi355_binary_asym_search``: the bits expanded to bytes in the kernel, the sums on the i8 MFMA).  The same codes, the same
  bytes, a finer order: over a thousand distinct scores per query where the symmetric search has 70-80 (D = 256), and refined
  recall@10 at a shortlist of 30 up from 0.78-0.83 to 0.88-0.92 on the tests' planted mixture.  ``bg.query_codes(queries)``
  returns the codes.

**The format is a shortlist generator.**  Its own top-k is coarse (at most ``dim + 1`` distinct scores; raw recall@10 of about
0.4 on a clustered mixture at D = 256), the refined search is what it is for.  **The centre is not optional for pooled
activations**: embeddings that are global-average pools of SiLU outputs are positive in nearly every element, so their raw sign
bits are all ones and every distance is 0 - ``train`` (or ``from_gallery``) first.  A rotation or a reduction in front of the
bits is the existing ``Whitening``: ``BinaryGallery(w.dim_out, device)`` fed with ``w.transform(x)`` (whitened rows are centred
and variance-balanced, so a zero centre serves them); no projection is built into the encoder.

The arithmetic is integer but for one fp32 division, and is specified bit for bit in include/mi355_retrieval.h; a NumPy model
(tests/binary_ref.py, tests/binary_asym_ref.py) reproduces every bit of the codes, the distances, the scores and the top-k.
Growth of the code buffer, labels, recall and the shortlist rules of ``refine=`` come from ``rank._RowStore``, as for the other
galleries.  Out of scope: an IVF index over binary codes, a sharded binary gallery, ITQ, more than one bit per
dimension, range search and the metric epilogues over codes.
"""
from __future__ import annotations

import torch

from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr

MAX_DIM = 65536
SCAN_CHUNK = 256                    # rows of one scan workgroup (BIN_CHUNK, csrc/binary.hip)
QUERY_BLOCK = 64                    # queries of one scan workgroup (BIN_QB)
ASYM_QUERY_BLOCK = 64               # queries of one asymmetric scan workgroup (BIN_AQB): two MFMA tiles of 32
SELECT_PASS = 32                    # queries of one pass of the in-kernel selection (BIN_QP)
SLICE_WORDS = 48                    # words of a row a lane holds at a time (BIN_SLICE): longer rows are scanned in slices


def words(dim: int) -> int:
    """Code words of a row: ``ceil(dim / 32)``."""
    return (int(dim) + 31) // 32


def row_words(dim: int) -> int:
    """Stored words of a row: ``words(dim)`` rounded up to a multiple of 4 (16 bytes)."""
    return (words(dim) + 3) & ~3


class BinaryGallery(_rank._RowStore):
    """Resident sign-bit gallery.  ``codes`` (rows, ceil(dim / 32)) int32: bit ``j % 32`` of word ``j / 32`` is 1 iff
    ``n[j] >= center[j]`` for the normalised row ``n``.  A search encodes its queries with the same centre and scores a row as
    ``(dim - 2 * popcount(q ^ g)) / dim``; order, ties, NaN queries and pads as ``cosine_topk``.  Ties (resolved to the lower
    row) are the normal case.  A row with a NaN element gets 0 bits where the NaN reaches: unlike the float galleries it does
    not rank first."""

    _NOUN = "BinaryGallery"
    _BUFFERS = ("_codes",)

    def __init__(self, dim: int, device, center: torch.Tensor | None = None, capacity: int = 0, eps: float = _rank._EPS):
        if not _rank._is_int(dim) or not 1 <= dim <= MAX_DIM:
            raise MI355Error(f"a BinaryGallery needs dim in [1, {MAX_DIM}], got {dim!r}")
        super().__init__(dim, device, eps)
        if self.device.type == "cuda" and self.device.index is None:       # "cuda": the index tensors on it report
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.W, self._ld = words(self.dim), row_words(self.dim)
        self._codes = torch.empty((max(int(capacity), 0), self._ld), dtype=torch.int32, device=self.device)
        self._center = None
        if center is not None:
            self._center = self._checked_center(center)

    def _checked_center(self, center) -> torch.Tensor:
        if not torch.is_tensor(center):
            raise MI355Error(f"center must be a ({self.dim},) fp32 tensor, got {type(center).__name__}")
        if center.device != self.device or tuple(center.shape) != (self.dim,):
            raise MI355Error(f"center must be ({self.dim},) on {self.device}, got {tuple(center.shape)} on {center.device}")
        return _rank._f32c(center, "center")

    # ---- training
    def train(self, rows) -> "BinaryGallery":
        """Sets ``center`` to the fp32 rounding of the float64 column mean of the normalised rows: ``rows`` is an fp32 device
        tensor (N, dim), N >= 1, normalised here, or an fp32 ``Gallery``.  The sums are ``embedding_moments``', whose order is
        fixed: the same bits on every run.  Refused once rows are resident: their codes were made with another centre and
        would be silently wrong."""
        from .whitening import embedding_moments
        if self.rows:
            raise MI355Error(f"train: {self.rows} rows are already resident (their codes belong to the present center)")
        if isinstance(rows, _rank.Gallery):
            if rows.dtype != torch.float32:
                raise MI355Error("train: an fp16 Gallery cannot train a BinaryGallery (training reads fp32 rows)")
            if rows.device != self.device or rows.dim != self.dim:
                raise MI355Error(f"train: the Gallery is ({rows.dim},) on {rows.device}, the BinaryGallery ({self.dim},) on "
                                 f"{self.device}")
            n, normalize = len(rows), False
        else:
            if not torch.is_tensor(rows):
                raise MI355Error(f"train: rows must be a tensor or a Gallery, got {type(rows).__name__}")
            if rows.dtype != torch.float32:
                raise MI355Error(f"train: rows must be fp32, got {rows.dtype}")
            if rows.dim() != 2 or rows.shape[1] != self.dim or rows.device != self.device:
                raise MI355Error(f"train: rows must be (N, {self.dim}) on {self.device}, got {tuple(rows.shape)} on {rows.device}")
            n, normalize = int(rows.shape[0]), True
        if n < 1:
            raise MI355Error("train: no rows to take a mean of")
        m = embedding_moments(rows, normalize=normalize, eps=self.eps)
        self._center = (m.sum / float(m.n)).to(torch.float32)
        return self

    @classmethod
    def from_gallery(cls, gallery) -> "BinaryGallery":
        """A BinaryGallery trained on the rows of an fp32 ``Gallery`` and holding them (and its labels)."""
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"from_gallery needs a Gallery, got {type(gallery).__name__}")
        bg = cls(gallery.dim, gallery.device, eps=gallery.eps).train(gallery)
        return bg._append(gallery.data, gallery.labels, normalized=True)

    # ---- the resident rows
    def _center_ptr(self):
        return None if self._center is None else self._center.data_ptr()

    def _encode(self, rows: torch.Tensor, normalized: bool, out: torch.Tensor) -> None:
        """Codes of the (n, dim) fp32 rows into ``out`` (n, row_words) int32, a slice of a code buffer."""
        n = rows.shape[0]
        with torch.cuda.device(self.device):
            check(lib().mi355_binary_encode(rows.data_ptr(), n, self.dim, int(normalized), self.eps, self._center_ptr(),
                                            out.data_ptr(), n * self._ld * 4, stream_ptr(self.device)))

    def _write(self, e: torch.Tensor, r0: int, normalized: bool) -> None:
        self._encode(e, normalized, self._codes[r0: r0 + e.shape[0]])

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None):
        e = self._new_rows(embeddings)
        if e.device != self.device:
            raise MI355Error(f"embeddings are on {e.device} but the gallery lives on {self.device}")
        return self._append(e, labels, normalized=False)

    @property
    def codes(self) -> torch.Tensor:
        """The (rows, ceil(dim / 32)) int32 code words (a view; the pad words of the stored rows are left out)."""
        return self._codes[: self.rows, : self.W]

    @property
    def center(self) -> torch.Tensor | None:
        """The (dim,) fp32 centre, or None (zeros) before ``train``."""
        return self._center

    @property
    def nbytes(self) -> int:
        """Resident footprint in bytes: the codes at the current capacity (``4 * row_words(dim)`` per row) and the centre."""
        return self._codes.shape[0] * self._ld * 4 + (0 if self._center is None else self.dim * 4)

    def _queries(self, queries: torch.Tensor, what: str) -> torch.Tensor:
        q = _rank._f32c(queries, "queries")
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise MI355Error(f"{what}: queries must be (Q, {self.dim}), got {tuple(q.shape)}")
        if q.device != self.device:
            raise MI355Error(f"{what}: queries are on {q.device} but the gallery lives on {self.device}")
        return q

    # ---- searching
    @staticmethod
    def _asym(asymmetric, what: str) -> bool:
        if not isinstance(asymmetric, bool):
            raise MI355Error(f"{what}: asymmetric must be a bool, got {asymmetric!r}")
        return asymmetric

    def distances(self, queries: torch.Tensor, asymmetric: bool = False) -> torch.Tensor:
        """(Q, rows) int32: the Hamming distance of every (query, row) pair, the integers ``search`` ranks by; the row of a
        query with a NaN is -1.  ``asymmetric=True``: the weighted distances ``m`` of the asymmetric search."""
        asym = self._asym(asymmetric, "distances")
        q = self._queries(queries, "distances")
        Q, G, L = q.shape[0], self.rows, lib()
        sizer, entry = (L.mi355_binary_asym_search_workspace_bytes, L.mi355_binary_asym_distances) if asym else \
            (L.mi355_binary_search_workspace_bytes, L.mi355_binary_distances)
        out = torch.empty((Q, G), dtype=torch.int32, device=self.device)
        if Q and G:
            ws = _rank._ws.get(self.device, sizer(Q, G, self.dim, 0))
            with torch.cuda.device(self.device):
                check(entry(q.data_ptr(), Q, self.dim, self.eps, self._center_ptr(), self._codes.data_ptr(), G,
                            out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(self.device)))
        return out

    def query_codes(self, queries: torch.Tensor):
        """(codes (Q, dim) int8, l1 (Q,) int32, nan (Q,) bool): what the asymmetric search makes of the queries - the int8 codes
        ``u`` of ``n - center``, ``sum |u|``, and whether the query is a NaN query (``mi355_binary_asym_query_codes``)."""
        q = self._queries(queries, "query_codes")
        Q = q.shape[0]
        codes = torch.empty((Q, self.dim), dtype=torch.int8, device=self.device)
        l1 = torch.empty((Q,), dtype=torch.int32, device=self.device)
        nan = torch.empty((Q,), dtype=torch.int32, device=self.device)
        if Q:
            with torch.cuda.device(self.device):
                check(lib().mi355_binary_asym_query_codes(q.data_ptr(), Q, self.dim, self.eps, self._center_ptr(), codes.data_ptr(),
                                                          l1.data_ptr(), nan.data_ptr(), stream_ptr(self.device)))
        return codes, l1, nan != 0

    def _bin_topk(self, q, k, idx_offset, filt, asym=False):
        Q, G, L = q.shape[0], self.rows, lib()
        sizer, entry = (L.mi355_binary_asym_search_workspace_bytes, L.mi355_binary_asym_search) if asym else \
            (L.mi355_binary_search_workspace_bytes, L.mi355_binary_search)
        vals = torch.empty((Q, k), dtype=torch.float32, device=self.device)
        idx = torch.empty((Q, k), dtype=torch.int64, device=self.device)
        if Q:
            ws = _rank._ws.get(self.device, sizer(Q, G, self.dim, k))
            with torch.cuda.device(self.device):
                check(entry(q.data_ptr(), Q, self.dim, self.eps, self._center_ptr(), self._codes.data_ptr(), G, k,
                            int(idx_offset), None if filt is None else filt[0], vals.data_ptr(), idx.data_ptr(),
                            ws.data_ptr(), ws.numel(), stream_ptr(self.device)))
        return vals, idx

    def search(self, queries: torch.Tensor, k: int, idx_offset: int = 0, *, query_labels: torch.Tensor | None = None,
               label_filter: str | None = None, exclude: torch.Tensor | None = None, refine=None, shortlist: int | None = None,
               asymmetric: bool = False):
        """(values (Q, k) fp32, indices (Q, k) int64), ``1 <= k <= min(1024, rows)``; filters and ``idx_offset`` as in
        ``Gallery.search``.  Without ``refine`` the values are the binary scores ``(dim - 2 h) / dim``.  With ``refine``, a
        ``Gallery`` (fp32 or fp16) of the same rows on the same device, the binary search returns ``shortlist`` rows per query
        (``k <= shortlist <= min(1024, rows)``, default ``min(max(10 * k, 100), 1024, rows)``), each is scored again as
        ``qn . row`` against the gallery's row (the bits an ``IVFIndex`` scan gives the pair) and the top-k of those values is
        returned.  Nothing is read back.  ``asymmetric=True`` scores the same codes against an int8 quantisation of
        ``n - center`` instead of the query's sign bits (``mi355_binary_asym_search``): the values are ``(L1 - 2 m) / L1`` with
        ``m`` the Hamming distance weighted by the query's magnitudes, a finer order and a better shortlist; everything else
        (filters, ``idx_offset``, ``refine``, ``shortlist``) is the same."""
        asym = self._asym(asymmetric, "search")
        k, R = self._shortlist_length(k, refine, shortlist)
        q = self._queries(queries, "search")
        Q = q.shape[0]
        gl = None if label_filter is None else self._labels_for(f'label_filter="{label_filter}"')
        filt = _rank._rank_filter(Q, self.rows, self.device, query_labels, gl, label_filter, exclude)
        vals, idx = self._bin_topk(q, R, idx_offset, filt, asym)
        if refine is None or Q == 0:
            return vals[:, :k], idx[:, :k]
        return self._refined_topk(q, vals, idx, k, refine, idx_offset)

    def recall(self, queries: torch.Tensor, k: int, exact: "_rank.Gallery", **search_kwargs):
        """(mean, per_query (Q,) float64): the share of ``exact.search(queries, k)``'s indices that ``search(queries, k,
        **search_kwargs)`` returns; ``exact`` is a ``Gallery`` of the same rows (pass ``refine=exact`` to measure the refined
        search, which is the one to measure: the format is a shortlist generator)."""
        return self._recall_against(exact, queries, k, **search_kwargs)
