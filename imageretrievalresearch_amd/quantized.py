"""8-bit resident gallery: scalar-quantised int8 rows with one fp32 scale per row, a quarter of the bytes of fp32 rows.

``Int8Gallery`` is a class of its own rather than a third ``dtype=`` of ``Gallery``: it carries extra state (the scales) and
offers part of ``Gallery``'s surface only - ``add``, ``search`` (filters included), ``range_search`` and ``recall``.  Its
searches go through the same ``_topk`` / ``_range`` as every other gallery (rank.py), so the workspace cache, the device
checks and the filter arguments are shared; the rows travel as a ``_Rows`` of dtype int8.  Growth of the two buffers, labels
and recall come from ``rank._RowStore``, the base it shares with ``Gallery`` and ``PQGallery``.

The format and its arithmetic are specified bit for bit in include/mi355_retrieval.h: the integer dot products are exact, so
a score depends on its query and its row alone - never on the number of queries, the kernel (GEMV or GEMM), its tiling or
the filter - and a small NumPy model (tests/gallery_i8_ref.py) reproduces every returned bit."""
from __future__ import annotations

import torch

from . import rank as _rank
from ._lib import MI355Error, check, lib, stream_ptr

_MAX_DIM = 65536       # the int32 dot products stay exact up to here
_SEGMENT = 128         # a stored row is a whole number of 128-byte segments


def _stride(dim: int) -> int:
    return (dim + _SEGMENT - 1) // _SEGMENT * _SEGMENT


class _ListIndexed:
    """``Int8Gallery.ivf``: the cached ``Int8IVFIndex`` (ivf_i8.py) over a gallery's codes.  It lives in a base of
    ``Int8Gallery`` as ``rank._GraphIndexed`` does for ``Gallery.graph``: the index is exported lazily and carries its own
    side-stream cases (tests/test_ivf_i8_gpu.py)."""

    def ivf(self, rows, nlist: int, **kw):
        """The ``Int8IVFIndex`` over these codes with ``nlist`` lists: ``Int8IVFIndex.build(self, rows, nlist, **kw)``
        (``iters``, ``seed``, ``init``); ``rows`` is the ``Gallery`` or the fp32 tensor the codes were made from.  Cached per
        (nlist, iters, seed) until ``add``; an index built from a given ``init`` is not cached."""
        from .ivf_i8 import Int8IVFIndex
        if kw.get("init") is not None:
            return Int8IVFIndex.build(self, rows, nlist, **kw)
        key = (nlist, kw.get("iters", 10), kw.get("seed", 0))
        if key not in self._ivf:
            self._ivf[key] = Int8IVFIndex.build(self, rows, nlist, **kw)
        return self._ivf[key]


class Int8Gallery(_rank._RowStore, _ListIndexed):
    """Resident int8 gallery.  A row is stored as ``codes = clamp(rint(n * 127 / amax), -127, 127)`` of its L2-normalised fp32
    row ``n`` (``amax = max |n_i|``) beside ``scale = amax / 127``: ``ld + 4`` bytes per row, ``ld`` = ``dim`` rounded up to a
    multiple of 128.  A search keeps about 15 bits of each query (two int8 planes), multiplies on the int8 matrix pipe and
    returns ``(acc_hi + acc_lo / 128) * s_q * s_g``; order, ties, NaN and pads as ``cosine_topk``.  The error against the
    fp32 cosine is that of the row quantisation, about 1e-3 at most and a few 1e-4 rms at the reference's widths: the
    top-k is approximate (``recall``)."""

    _NOUN = "Int8Gallery"

    def __init__(self, dim: int, device, capacity: int = 0, eps: float = _rank._EPS):
        super().__init__(dim, device, eps)
        if not 1 <= self.dim <= _MAX_DIM:
            raise MI355Error(f"an Int8Gallery needs 1 <= dim <= {_MAX_DIM}, got {dim}")
        self._ld = _stride(self.dim)
        cap = max(int(capacity), 0)
        self._codes = torch.empty((cap, self._ld), dtype=torch.int8, device=self.device)
        self._scales = torch.empty((cap,), dtype=torch.float32, device=self.device)
        self._ivf = {}                                           # per (nlist, iters, seed); dropped by add

    _BUFFERS = ("_codes", "_scales")

    def _write(self, e: torch.Tensor, r0: int, normalized: bool) -> None:
        n = e.shape[0]
        codes, scales = self._codes[r0: r0 + n], self._scales[r0: r0 + n]
        with torch.cuda.device(e.device):
            check(lib().mi355_gallery_to_i8(e.data_ptr(), n, self.dim, int(normalized), self.eps, codes.data_ptr(),
                                            n * self._ld, scales.data_ptr(), stream_ptr(e.device)))

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None):
        self._ivf = {}
        return self._append(self._new_rows(embeddings), labels, normalized=False)

    @property
    def codes(self) -> torch.Tensor:
        """The (rows, dim) int8 codes (a view, without the row padding)."""
        return self._codes[: self.rows, : self.dim]

    @property
    def scales(self) -> torch.Tensor:
        """The (rows,) fp32 scales (a view)."""
        return self._scales[: self.rows]

    def dequantized(self) -> torch.Tensor:
        """(rows, dim) fp32: ``codes.float() * scales[:, None]``."""
        return self.codes.float() * self.scales[:, None]

    @property
    def nbytes(self) -> int:
        """Resident footprint in bytes: codes and scales at the current capacity, ``capacity * (ld + 4)``."""
        return self._codes.shape[0] * (self._ld + 4)

    def _resident(self) -> _rank._Rows:
        return _rank._Rows(self._codes, self.rows, self.dim, True, None, self._scales)

    def search(self, queries: torch.Tensor, k: int, idx_offset: int = 0, *, query_labels: torch.Tensor | None = None,
               label_filter: str | None = None, exclude: torch.Tensor | None = None, refine=None, shortlist: int | None = None):
        """Top-k of ``queries`` against the resident rows, arguments and result as ``Gallery.search`` (without ``qe``).
        ``refine`` / ``shortlist`` as in ``PQGallery.search``: with ``refine``, a ``Gallery`` (fp32 or fp16) of the same rows on
        the same device, the int8 search returns ``shortlist`` rows per query (``k <= shortlist <= min(1024, rows)``, default
        ``min(max(10 * k, 100), 1024, rows)``), each is scored again as ``qn . row`` against the gallery's row (the bits an
        ``IVFIndex`` scan gives the pair) and the top-k of those values is returned."""
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

    def recall(self, queries: torch.Tensor, k: int, exact: "_rank.Gallery"):
        """(mean, per_query (Q,) float64): the share of ``exact.search(queries, k)``'s indices that ``search(queries, k)``
        returns; ``exact`` is a ``Gallery`` of the same rows."""
        return self._recall_against(exact, queries, k)
