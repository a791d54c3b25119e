"""4-bit resident gallery: e2m1 rows, two codes per byte, with one fp32 multiplier per row - half the bytes of int8 rows - searched
on the block-scaled fp4 matrix instruction of gfx950 (``v_mfma_scale_f32_32x32x64_f8f6f4``), which reads the packed nibbles as
they lie in memory.

``FP4Gallery`` sits between ``Int8Gallery`` (8 bits per dimension) and ``BinaryGallery`` (1 bit) and is patterned on the
former: ``add``, ``search`` (filters, ``refine=`` / ``shortlist=``), ``range_search`` and ``recall``, through the same ``_topk`` /
``_range`` as every other gallery (rank.py); the rows travel as a ``_Rows`` of dtype uint8.  Growth of the two buffers, labels,
recall and the shortlist rules come from ``rank._RowStore``.

The format and its arithmetic are specified bit for bit in include/mi355_retrieval.h: every partial sum of a dot product is a
multiple of 0.25 that fp32 holds exactly, so a score depends on its query and its row alone - never on the number of queries,
the kernel (GEMV or GEMM), its tiling or the filter - and a small NumPy model (tests/gallery_fp4_ref.py) reproduces every
returned bit."""
from __future__ import annotations

import torch

from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr

_MAX_DIM = 65536       # the fp32 sums of multiples of 0.25 stay exact up to here
_SEGMENT = 128         # a stored row is a whole number of 128-byte segments


def _stride(dim: int) -> int:
    return ((dim + 1) // 2 + _SEGMENT - 1) // _SEGMENT * _SEGMENT


class FP4Gallery(_rank._RowStore):
    """Resident fp4 gallery.  A row is stored as ``codes = e2m1(n * 6 / amax)`` of its L2-normalised fp32 row ``n`` (``amax = max
    |n_i|``; e2m1: sign and one of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, nearest, ties to even), dimension ``2j`` in the low nibble of
    byte ``j``, beside ``mult = 1 / |value(codes)|``: ``ld + 4`` bytes per row, ``ld`` = ``ceil(dim / 2)`` rounded up to a multiple
    of 128 (772 B at dim 1536).  A search splits each query into two e2m1 planes, multiplies on the fp4 matrix pipe and returns
    ``(acc_hi + acc_lo / 4) * s_q * mult``; order, ties, NaN and pads as ``cosine_topk``.  Four bits keep a few per cent of error
    against the fp32 cosine: the top-k is approximate (``recall``), and ``refine=`` rescores a shortlist exactly."""

    _NOUN = "FP4Gallery"

    def __init__(self, dim: int, device, capacity: int = 0, eps: float = _rank._EPS):
        super().__init__(dim, device, eps)
        if not 1 <= self.dim <= _MAX_DIM:
            raise MI355Error(f"an FP4Gallery needs 1 <= dim <= {_MAX_DIM}, got {dim}")
        self._ld = _stride(self.dim)
        cap = max(int(capacity), 0)
        self._codes = torch.empty((cap, self._ld), dtype=torch.uint8, device=self.device)
        self._mults = torch.empty((cap,), dtype=torch.float32, device=self.device)

    _BUFFERS = ("_codes", "_mults")

    def _write(self, e: torch.Tensor, r0: int, normalized: bool) -> None:
        n = e.shape[0]
        codes, mults = self._codes[r0: r0 + n], self._mults[r0: r0 + n]
        with torch.cuda.device(e.device):
            check(lib().mi355_gallery_to_fp4(e.data_ptr(), n, self.dim, int(normalized), self.eps, codes.data_ptr(),
                                             n * self._ld, mults.data_ptr(), stream_ptr(e.device)))

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None):
        return self._append(self._new_rows(embeddings), labels, normalized=False)

    @classmethod
    def from_gallery(cls, gallery: "_rank.Gallery") -> "FP4Gallery":
        """An ``FP4Gallery`` of the resident rows of an fp32 ``Gallery``: the rows are normalised already, so its codes and
        multipliers are bit for bit those of ``add`` of the original embeddings.  Labels are copied."""
        if not isinstance(gallery, _rank.Gallery) or gallery.dtype != torch.float32:
            raise MI355Error("FP4Gallery.from_gallery makes fp4 codes of the fp32 rows of a Gallery; quantise other embeddings with add")
        out = cls(gallery.dim, gallery.device, capacity=gallery.rows, eps=gallery.eps)
        out._append(gallery.data, None if gallery.labels is None else gallery.labels.clone(), normalized=True)
        return out

    @property
    def codes(self) -> torch.Tensor:
        """The (rows, ceil(dim / 2)) packed uint8 codes (a view, without the row padding): dimension 2j in the low nibble of
        byte j."""
        return self._codes[: self.rows, : (self.dim + 1) // 2]

    @property
    def mults(self) -> torch.Tensor:
        """The (rows,) fp32 multipliers (a view)."""
        return self._mults[: self.rows]

    def dequantized(self) -> torch.Tensor:
        """(rows, dim) fp32 unit rows: ``value(code) * mult``."""
        c = self.codes
        nib = torch.stack((c & 15, c >> 4), dim=2).reshape(self.rows, -1)[:, : self.dim]
        m = (nib & 7).float()                                    # magnitudes 0, 0.5, 1, 1.5, 2 | 3, 4 | 6, without a host table
        mag = torch.where(m < 5, 0.5 * m, torch.where(m < 7, m - 2.0, 6.0))
        return torch.where(nib >= 8, -mag, mag) * self.mults[:, None]

    @property
    def nbytes(self) -> int:
        """Resident footprint in bytes: codes and multipliers at the current capacity, ``capacity * (ld + 4)``."""
        return self._codes.shape[0] * (self._ld + 4)

    def _resident(self) -> _rank._Rows:
        return _rank._Rows(self._codes, self.rows, self.dim, True, None, self._mults)

    def search(self, queries: torch.Tensor, k: int, idx_offset: int = 0, *, query_labels: torch.Tensor | None = None,
               label_filter: str | None = None, exclude: torch.Tensor | None = None, refine=None, shortlist: int | None = None):
        """Top-k of ``queries`` against the resident rows, arguments and result as ``Int8Gallery.search``: with ``refine``, a
        ``Gallery`` (fp32 or fp16) of the same rows on the same device, the fp4 search returns ``shortlist`` rows per query
        (``k <= shortlist <= min(1024, rows)``, default ``min(max(10 * k, 100), 1024, rows)``), each is scored again as
        ``qn . row`` against the gallery's row and the top-k of those values is returned."""
        gl = None if label_filter is None else self._labels_for(f'label_filter="{label_filter}"')
        if refine is None and shortlist is None:
            return _rank._topk(queries, self._resident(), k, self.eps, idx_offset, query_labels, gl, label_filter, exclude)
        k, R = self._shortlist_length(k, refine, shortlist)
        q = _rank._f32c(queries, "queries")
        vals, idx = _rank._topk(q, self._resident(), R, self.eps, idx_offset, query_labels, gl, label_filter, exclude)
        if q.shape[0] == 0:
            return vals[:, :k], idx[:, :k]
        return self._refined_topk(q, vals.contiguous(), idx.contiguous(), k, refine, idx_offset)

    def range_search(self, queries: torch.Tensor, threshold: float, *, query_labels: torch.Tensor | None = None,
                     label_filter: str | None = None, exclude: torch.Tensor | None = None, max_results: int | None = None,
                     idx_offset: int = 0) -> _rank.RangeResult:
        """Every row whose score is >= ``threshold``, arguments and result as ``Gallery.range_search``; the scores are the
        bits ``search`` returns for the same pair."""
        gl = None if label_filter is None else self._labels_for(f'label_filter="{label_filter}"')
        return _rank._range(queries, self._resident(), threshold, self.eps, idx_offset, query_labels, gl, label_filter, exclude,
                            max_results)

    def recall(self, queries: torch.Tensor, k: int, exact: "_rank.Gallery", **search_kwargs):
        """(mean, per_query (Q,) float64): the share of ``exact.search(queries, k)``'s indices that ``search(queries, k,
        **search_kwargs)`` returns (``refine=`` / ``shortlist=``); ``exact`` is a ``Gallery`` of the same rows."""
        return self._recall_against(exact, queries, k, **search_kwargs)
