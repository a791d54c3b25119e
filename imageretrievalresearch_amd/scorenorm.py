"""Corrections of the cosine score itself (the reference ranks and thresholds the raw cosine): CSLS against hubness (Conneau et
al., ICLR 2018) and cohort normalisation for verification (Z-, T-, S-norm and, with a top-n cohort, adaptive S-norm).

Both are one affine map of the score with per-query and per-gallery-row coefficients, applied inside the cosine GEMM
(csrc/rank_common.h, definitions in include/mi355_retrieval.h): ``t = s * (aq[q] + ag[g]) - (bq[q] + bg[g])`` in fp32 without
fused multiply-add, in front of the fused per-tile selection, so that a search over ``t`` needs no Q x G slab.

* ``adjusted_topk`` / ``adjusted_scores`` ... the low-level forms: any coefficient vectors  (mi355_rank_topk_adjusted[_f16],
                                               mi355_cosine_scores_adjusted[_f16])
* ``neighbourhood_stats`` ................... mean, deviation and count of each row's n largest cosines against a cohort: the
                                               existing search, then mi355_topn_stats
* ``ScoreNorm`` ............................. the gallery side's coefficients, fitted once, and the rule for the query side;
                                               ``Gallery.score_norm`` builds one, ``Gallery.search_normed`` searches with it

| kind    | gallery side (rows against the cohort)  | query side                                                         |
| "csls"  | bg = mean of the top n (n = 10)         | aq = 2, bq = mean of the query's top n against the gallery         |
| "znorm" | ag = 1 / std, bg = mean / std           | none                                                               |
| "tnorm" | none                                    | aq = 1 / std, bq = mean / std of the query's top n against cohort  |
| "snorm" | half of z                               | half of t                                                          |

For the three norms ``n=None`` takes the whole cohort and a given ``n`` is the adaptive variant.  Only the finite check of the
fitted coefficients reads a result back to the host.  Out of scope (INTEGRATION.md names the follow-ups): ``ShardedGallery``, the
int8, fp4, PQ and binary galleries, the list and graph indexes, range search and ``verification_roc`` under adjusted scores."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import MI355Error, ScoreAdjust, check, lib, require_cuda, stream_ptr
from .rank import _EPS, _MAX_K, Gallery, _check_qg, _f32c, _is_int, _rank_filter, _Rows, _topk, _ws, l2_normalize_rows

KINDS = ("csls", "znorm", "tnorm", "snorm")
CSLS_N = 10

_ENTRIES = {torch.float32: ("mi355_rank_topk_adjusted", "mi355_cosine_scores_adjusted", "mi355_rank_adjusted_workspace_bytes"),
            torch.float16: ("mi355_rank_topk_adjusted_f16", "mi355_cosine_scores_adjusted_f16",
                            "mi355_rank_adjusted_f16_workspace_bytes")}


def _coefficient(t, name: str, n: int):
    """None, or a coefficient vector as the kernels read it: float32, shape (n,).  Checked before any device is touched."""
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise MI355Error(f"{name} must be None or a float32 tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise MI355Error(f"{name} must be float32, got {t.dtype}")
    if t.dim() != 1 or t.shape[0] != n:
        raise MI355Error(f"{name} must have shape ({n},), got {tuple(t.shape)}")
    return t


def _coefficients(Q: int, G: int, aq, bq, ag, bg):
    co = (_coefficient(aq, "aq", Q), _coefficient(bq, "bq", Q), _coefficient(ag, "ag", G), _coefficient(bg, "bg", G))
    if co[0] is None and co[2] is None:
        raise MI355Error("at least one of aq and ag must be given (the score's factor would be 0 everywhere)")
    return co


def _on(t, name: str, device):
    if t is None:
        return None
    require_cuda(t, name)
    if t.device != torch.device(device):
        raise MI355Error(f"{name} is on {t.device} but the search runs on {device}")
    return t.contiguous()


def _rows_of(gallery, normalized: bool = False) -> _Rows:
    """The fp32 or fp16 rows of a ``Gallery`` (the planes of ``prepare()`` are not used: an adjusted search of a prepared gallery
    runs on its fp32 rows, as a filtered one does), of a ``_Rows`` or of a (G, D) tensor."""
    if isinstance(gallery, Gallery):
        return _Rows(gallery._buf, gallery.rows, gallery.dim, True)
    if isinstance(gallery, _Rows) or torch.is_tensor(gallery):
        r = _Rows.of(gallery, normalized)
        if r.buf is None or r.dtype not in _ENTRIES:
            raise MI355Error("adjusted scores read fp32 or fp16 rows; these rows are not supported")
        return _Rows(r.buf, r.rows, r.dim, r.normalized)
    raise MI355Error(f"adjusted scores read the fp32 or fp16 rows of a Gallery or a (G, D) tensor; a {type(gallery).__name__} is not "
                     "supported")


def _shapes(queries, gallery):
    """(Q, G) of a call, read off the arguments before any of them has to be on a device."""
    if not torch.is_tensor(queries) or queries.dim() != 2:
        raise MI355Error("expected (Q,D) queries")
    if isinstance(gallery, (Gallery, _Rows)):
        return queries.shape[0], gallery.rows
    if torch.is_tensor(gallery) and gallery.dim() == 2:
        return queries.shape[0], gallery.shape[0]
    raise MI355Error(f"adjusted scores read the fp32 or fp16 rows of a Gallery or a (G, D) tensor; a {type(gallery).__name__} is not "
                     "supported")


def _query_block(query_block) -> int:
    if not _is_int(query_block) or int(query_block) < 0:
        raise MI355Error(f"query_block must be an integer >= 0 (0: the default rule), got {query_block!r}")
    return int(query_block)


def _adjust(dev, co):
    a = ScoreAdjust()
    keep = [_on(t, n, dev) for t, n in zip(co, ("aq", "bq", "ag", "bg"))]
    a.aq, a.bq, a.ag, a.bg = (None if t is None else t.data_ptr() for t in keep)
    return a, keep


def _adjusted_topk(queries, rows: _Rows, k, co, idx_offset=0, query_labels=None, gallery_labels=None, label_filter=None, exclude=None,
                   query_block=0, eps=_EPS):
    if not _is_int(k) or not 1 <= int(k) <= min(rows.rows, _MAX_K):
        raise MI355Error(f"selected index k out of range: k={k!r}, gallery rows={rows.rows} (at most {_MAX_K})")
    k, qb = int(k), _query_block(query_block)
    q = _f32c(queries, "queries")
    _check_qg(q, rows)
    Q, G, dev = q.shape[0], rows.rows, q.device
    adj, keep = _adjust(dev, co)
    filt = _rank_filter(Q, G, dev, query_labels, gallery_labels, label_filter, exclude)
    vals = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    if Q == 0:
        return vals, idx
    L = lib()
    entry, _, sizer = _ENTRIES[rows.dtype]
    ws = _ws.get(dev, getattr(L, sizer)(Q, G, rows.dim, k))
    with torch.cuda.device(dev):
        check(getattr(L, entry)(q.data_ptr(), Q, *rows.c_args(), k, eps, int(idx_offset), C.byref(adj),
                                None if filt is None else C.byref(filt[0]), qb, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                ws.numel(), stream_ptr(dev)))
    return vals, idx


def _adjusted_scores(queries, rows: _Rows, co, query_block=0, eps=_EPS):
    qb = _query_block(query_block)
    q = _f32c(queries, "queries")
    _check_qg(q, rows)
    Q, G, dev = q.shape[0], rows.rows, q.device
    adj, keep = _adjust(dev, co)
    out = torch.empty((Q, G), dtype=torch.float32, device=dev)
    if Q == 0 or G == 0:
        return out
    L = lib()
    _, entry, sizer = _ENTRIES[rows.dtype]
    ws = _ws.get(dev, getattr(L, sizer)(Q, G, rows.dim, 0))
    with torch.cuda.device(dev):
        check(getattr(L, entry)(q.data_ptr(), Q, *rows.c_args(), eps, C.byref(adj), qb, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                stream_ptr(dev)))
    return out


def adjusted_topk(queries: torch.Tensor, gallery, k: int, *, aq=None, bq=None, ag=None, bg=None, eps: float = _EPS,
                  gallery_is_normalized: bool = False, query_labels=None, gallery_labels=None, label_filter=None, exclude=None,
                  idx_offset: int = 0, query_block: int = 0):
    """Top-k of ``t = s * (aq[q] + ag[g]) - (bq[q] + bg[g])`` (fp32, no fused multiply-add; a vector left out counts as 0, one of
    ``aq`` / ``ag`` is needed), ``s`` the cosine of the pair as the tiled GEMM of the rows gives it.  ``gallery``: a (G, D) tensor,
    a ``Gallery`` (fp32 or fp16) or its rows.  Returns (t values (Q, k) fp32, indices (Q, k) int64): descending t, ties to the lower
    index, NaN first; the filter arguments and ``idx_offset`` as in ``cosine_topk``.  ``query_block``: at most that many queries
    per GEMM call (0: the library's rule; results do not depend on it)."""
    Q, G = _shapes(queries, gallery)
    co = _coefficients(Q, G, aq, bq, ag, bg)
    if not _is_int(k) or not 1 <= int(k) <= min(G, _MAX_K):
        raise MI355Error(f"selected index k out of range: k={k!r}, gallery rows={G} (at most {_MAX_K})")
    _query_block(query_block)
    rows = _rows_of(gallery, gallery_is_normalized)
    if isinstance(gallery, Gallery) and gallery_labels is None and label_filter is not None:
        gallery_labels = gallery._labels_for(f'label_filter="{label_filter}"')
    return _adjusted_topk(queries, rows, k, co, idx_offset, query_labels, gallery_labels, label_filter, exclude, query_block, eps)


def adjusted_scores(queries: torch.Tensor, gallery, *, aq=None, bq=None, ag=None, bg=None, eps: float = _EPS,
                    gallery_is_normalized: bool = False, query_block: int = 0) -> torch.Tensor:
    """The (Q, G) fp32 slab of ``t`` (see ``adjusted_topk``): element for element the values a search over it returns."""
    Q, G = _shapes(queries, gallery)
    co = _coefficients(Q, G, aq, bq, ag, bg)
    _query_block(query_block)
    return _adjusted_scores(queries, _rows_of(gallery, gallery_is_normalized), co, query_block, eps)


def _cohort_n(n, cohort_rows: int, default=None) -> int:
    """The neighbourhood size: ``n`` (None: ``default``, or the whole cohort) within [1, min(cohort rows, 1024)]."""
    top = min(cohort_rows, _MAX_K)
    if n is None:
        n = cohort_rows if default is None else min(default, top)
    if not _is_int(n) or not 1 <= int(n) <= top:
        raise MI355Error(f"n must be an integer in [1, min(cohort rows, {_MAX_K})] = [1, {top}] (None: the whole cohort, when it has at "
                         f"most {_MAX_K} rows), got {n!r} for {cohort_rows} cohort rows")
    return int(n)


def _min_std(min_std) -> float:
    try:
        m = float(min_std)
    except (TypeError, ValueError):
        raise MI355Error(f"min_std must be a finite float >= 0, got {min_std!r}") from None
    if isinstance(min_std, bool) or not np.isfinite(m) or m < 0:
        raise MI355Error(f"min_std must be a finite float >= 0, got {min_std!r}")
    return m


def topn_stats(vals: torch.Tensor, idx: torch.Tensor, half: float | None = None, min_std: float = 1e-6):
    """(mean (N,) fp32, std (N,) fp32, count (N,) int32) of the real entries (index >= 0) of each row of a top-n result
    ``vals`` / ``idx`` (N, n): float64 sums in slot order, the population deviation, rounded once; a row without a real entry
    gives (0, 0, 0).  With ``half`` two more vectors follow: ``a = half / max(std, min_std)`` and ``b = mean * a``, computed in
    float64 (the coefficients of a cohort normalisation)."""
    require_cuda(vals, "vals")
    if (not torch.is_tensor(idx) or idx.dtype != torch.int64 or vals.dtype != torch.float32 or vals.dim() != 2
            or idx.shape != vals.shape or idx.device != vals.device):
        raise MI355Error("topn_stats expects float32 values and int64 indices of one (N, n) shape on one device")
    N, n = vals.shape
    if not 1 <= n <= _MAX_K:
        raise MI355Error(f"n={n} outside [1, {_MAX_K}]")
    vals, idx, dev = vals.contiguous(), idx.contiguous(), vals.device
    mean, std = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    ab = () if half is None else (torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev))
    if N:
        with torch.cuda.device(dev):
            check(lib().mi355_topn_stats(vals.data_ptr(), idx.data_ptr(), N, n, 1.0 if half is None else float(half), _min_std(min_std),
                                         mean.data_ptr(), std.data_ptr(), count.data_ptr(),
                                         *([t.data_ptr() for t in ab] or [None, None]), stream_ptr(dev)))
    return (mean, std, count) + ab


def _stats_against(rows: torch.Tensor, cohort: _Rows, n: int, exclude=None, half=None, min_std=1e-6, eps=_EPS):
    vals, idx = _topk(rows, cohort, n, eps, 0, None, None, None, exclude)
    return topn_stats(vals, idx, half, min_std)


def neighbourhood_stats(rows: torch.Tensor, cohort, n: int | None = None, *, exclude=None, eps: float = _EPS):
    """(mean, std, count) of each row's ``n`` largest cosines against ``cohort`` (a (C, D) tensor, a ``Gallery`` or its rows):
    the existing search with ``rows`` as the queries (``n`` > 8: through the score slab), then ``topn_stats``.  ``n=None`` is the
    whole cohort; 1 <= n <= min(cohort rows, 1024).  ``exclude`` (rows,) int64 leaves one cohort row out per row - the row itself,
    for a cohort that contains the rows."""
    co = _rows_of(cohort)
    return _stats_against(rows, co, _cohort_n(n, co.rows), exclude, eps=eps)


class ScoreNorm:
    """A fitted score normalisation: the gallery side's coefficients ``ag`` / ``bg`` (fp32, one per gallery row, checked finite
    once here) and the rule for the query side (see the module's table).  It belongs to the gallery it was fitted on, at the
    row count it had then: a gallery that has grown since raises, fit again."""

    def __init__(self, kind: str, rows: int, *, n=None, min_std: float = 1e-6, ag=None, bg=None, cohort: _Rows | None = None):
        if kind not in KINDS:
            raise MI355Error(f"kind must be one of {KINDS}, got {kind!r}")
        if not _is_int(rows) or int(rows) < 1:
            raise MI355Error(f"a ScoreNorm needs a gallery with rows, got rows={rows!r}")
        self.kind, self.rows, self.min_std = kind, int(rows), _min_std(min_std)
        self.ag, self.bg = _coefficient(ag, "ag", self.rows), _coefficient(bg, "bg", self.rows)
        need = {"csls": (False, True), "znorm": (True, True), "tnorm": (False, False), "snorm": (True, True)}[kind]
        if (self.ag is not None, self.bg is not None) != need:
            raise MI355Error(f'kind="{kind}" holds ' + " and ".join(x for x, on in zip(("ag", "bg"), need) if on) +
                             (" only" if any(need) else "no gallery side"))
        if kind in ("tnorm", "snorm") and cohort is None:
            raise MI355Error(f'kind="{kind}" needs the cohort rows for the query side')
        self.cohort = cohort
        top = self.rows if kind == "csls" else cohort.rows if cohort is not None else _MAX_K
        self.n = _cohort_n(n, top, CSLS_N if kind == "csls" else None)
        for name, t in (("ag", self.ag), ("bg", self.bg)):
            if t is not None and not bool(torch.isfinite(t).all()):          # the one read-back
                raise MI355Error(f"{name} has a non-finite coefficient (a NaN row, or min_std=0 with a constant neighbourhood)")
        self.half = 0.5 if kind == "snorm" else 1.0

    @classmethod
    def fit(cls, gallery: Gallery, cohort, kind: str = "csls", n=None, min_std: float = 1e-6) -> "ScoreNorm":
        """The gallery side from each resident row's ``n`` largest cosines against ``cohort`` ((C, D) tensor or ``Gallery``:
        samples of the query domain for "csls", impostors for the norms).  "csls": n = 10 by default, also the size of the query's
        neighbourhood in the gallery; the norms: None is the whole cohort (at most 1024 rows), a given n the adaptive variant."""
        if kind not in KINDS:
            raise MI355Error(f"kind must be one of {KINDS}, got {kind!r}")
        if not isinstance(gallery, Gallery):
            raise MI355Error(f"a ScoreNorm is fitted on a Gallery (fp32 or fp16 rows); a {type(gallery).__name__} is not supported")
        if gallery.rows < 1:
            raise MI355Error("the gallery holds no rows")
        co = _rows_of(cohort)
        if isinstance(cohort, torch.Tensor):                       # normalised once here: the query side searches it per batch
            co = _Rows(l2_normalize_rows(co.buf, gallery.eps), co.rows, co.dim, True)
        n = _cohort_n(n, min(co.rows, gallery.rows) if kind == "csls" else co.rows, CSLS_N if kind == "csls" else None)
        min_std = _min_std(min_std)
        ag = bg = None
        if kind != "tnorm":
            half = 0.5 if kind == "snorm" else 1.0
            mean, _, _, a, b = _stats_against(gallery.data, co, n, None, half, min_std, gallery.eps)
            ag, bg = (None, mean) if kind == "csls" else (a, b)
        return cls(kind, gallery.rows, n=n, min_std=min_std, ag=ag, bg=bg, cohort=None if kind in ("csls", "znorm") else co)

    def _check(self, gallery) -> Gallery:
        if not isinstance(gallery, Gallery):
            raise MI355Error(f"a ScoreNorm applies to the Gallery it was fitted on; a {type(gallery).__name__} is not supported")
        if gallery.rows != self.rows:
            raise MI355Error(f"this ScoreNorm was fitted on {self.rows} gallery rows, the gallery now holds {gallery.rows}: fit again "
                             "(Gallery.score_norm)")
        return gallery

    def query_side(self, gallery: Gallery, queries: torch.Tensor, idx_offset: int = 0, **filt):
        """(aq, bq) of a batch of queries, or (None, None) for "znorm".  "csls" searches the gallery with the filter arguments of
        the search itself (a leave-one-out search never counts the query's own row), the norms search the cohort."""
        gallery = self._check(gallery)
        if self.kind == "znorm":
            return None, None
        if self.kind == "csls":
            vals, idx = gallery.search(queries, self.n, idx_offset, **filt)
            mean = topn_stats(vals, idx)[0]
            return torch.full_like(mean, 2.0), mean
        q = _f32c(queries, "queries")
        _check_qg(q, self.cohort)
        return _stats_against(q, self.cohort, self.n, None, self.half, self.min_std, gallery.eps)[3:]

    def search(self, gallery: Gallery, queries: torch.Tensor, k: int, idx_offset: int = 0, *, query_labels=None, label_filter=None,
               exclude=None, query_block: int = 0):
        gallery = self._check(gallery)
        filt = dict(query_labels=query_labels, label_filter=label_filter, exclude=exclude)
        aq, bq = self.query_side(gallery, queries, idx_offset, **filt)
        gl = None if label_filter is None else gallery._labels_for(f'label_filter="{label_filter}"')
        return _adjusted_topk(queries, _rows_of(gallery), k, (aq, bq, self.ag, self.bg), idx_offset, query_labels, gl, label_filter,
                              exclude, query_block, gallery.eps)

    def scores(self, gallery: Gallery, queries: torch.Tensor) -> torch.Tensor:
        """The (Q, G) slab of normalised scores: with ``roc_curve`` it covers small verification sets."""
        gallery = self._check(gallery)
        aq, bq = self.query_side(gallery, queries)
        return _adjusted_scores(queries, _rows_of(gallery), (aq, bq, self.ag, self.bg), 0, gallery.eps)
