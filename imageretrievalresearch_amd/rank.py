"""Host side of the rank half: cosine similarity, top-k, ContrastiveLoss, retrieval metrics.

Mirrors the torch objects the reference uses (same names, argument meaning, error behaviour) and
routes the arithmetic to libmi355_retrieval:

* ``CosineSimilarity(dim=1, eps=1e-6)`` ....... train/train.py:73, inference/inference.py:169
* ``topk(sim, k)`` ............................ train/train.py:251,356 ; notebook raw :238
* ``cosine_topk(Q, G, k)`` .................... the whole per-query loop train/train.py:249-255 as one call
* ``ContrastiveLoss(margin)(fm1, fm2, label, mean)`` ... utils/contrastive_loss.py:6-61
* ``hit_counts`` / ``distinct_class_topn`` .... train/train.py:252-255 ; notebook raw :240-251
* ``roc_curve`` / ``verification_roc`` ........ utils/roc_curve_from_scratch.py (given pair scores / every labelled pair)
* ``cosine_range`` ............................ the pairs a verification threshold accepts (``score >= threshold``)
* ``positive_ranks`` / ``ranking_metrics`` .... full-gallery rank of every positive, mAP and CMC (not in the reference)
* ``expand_queries`` / ``Gallery.augmented`` .. alpha query expansion and database-side augmentation (not in the reference)
* ``Gallery.moments`` / ``Gallery.whitened`` .. PCA whitening of a resident gallery (whitening.py; not in the reference)
* ``Gallery.rerank`` / ``Gallery.rerank_index`` k-reciprocal re-ranking on the gallery's kNN graph (rerank.py; not in the reference)
* ``Gallery.kmeans`` / ``Gallery.clustering_metrics`` spherical k-means, NMI / purity / F1 (cluster.py; not in the reference)

The gallery side of every search is one ``_Rows`` (buffer, dtype, rows, dim, row stride, normalised or not, optional bf16
planes): a tensor argument, a ``PreparedGallery``, a ``Gallery`` and a ``ShardedGallery`` shard all become one.  Top-k, range
and ROC histogram are one function each (``_topk``, ``_range``, ``_roc_hist``) that checks the arguments once and picks the
fp32, fp16 or int8 C entry from ``_ENTRIES``; the public functions and methods are wrappers that add their own labels.  (int8 rows
come from an ``Int8Gallery``, quantized.py, and have the top-k and range entries only.)  ``Gallery``, ``Int8Gallery`` and
``PQGallery`` (pq.py) grow their buffers, keep their labels, measure recall and rescore a ``refine=`` shortlist through one base,
``_RowStore``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from ._lib import (DTYPE_F16, DTYPE_F32, LABEL_ANY, LABEL_DIFFERENT, LABEL_SAME, MI355Error, RankFilter, check, lib,
                   require_cuda, stream_ptr)

_EPS = 1e-6


def _is_int(x) -> bool:
    """An integer argument: a Python or NumPy integer, never a bool."""
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    require_cuda(t, name)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class _Workspace:
    """Scratch that only grows, one buffer per (device, stream): calls issued on different streams (bench.py runs the rank
    beside the embed) never share a workspace, and a buffer that is replaced by a bigger one is handed back to torch's
    caching allocator on the stream that used it (``record_stream``), so it is not recycled under a running kernel."""

    def __init__(self):
        self.buf = {}

    def get(self, device, nbytes: int) -> torch.Tensor:
        device = torch.device(device)
        stream = torch.cuda.current_stream(device)
        key = (device, stream.cuda_stream)
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            if b is not None:
                b.record_stream(stream)
            with torch.cuda.stream(stream):
                b = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b


_ws = _Workspace()


def _retire(old: torch.Tensor | None, device) -> None:
    """A resident buffer that was just replaced (a queued copy or ``torch.cat`` on the current stream still reads it): tell the
    caching allocator, as ``_Workspace.get`` does, so that its block is not handed out again - on the stream that allocated
    it, which need not be this one - before that read has run."""
    if old is not None and old.is_cuda and old.numel():
        old.record_stream(torch.cuda.current_stream(device))


def synth_fill(n: int, seed: int, kind: int, device, offset: int = 0) -> torch.Tensor:
    """Device-side portable generator (bit-identical to ``synth.fill``)."""
    out = torch.empty(int(n), dtype=torch.float32, device=device)
    require_cuda(out, "synth_fill output")
    with torch.cuda.device(out.device):
        check(lib().mi355_synth_fill(out.data_ptr(), int(n), int(seed), int(offset), int(kind),
                                     stream_ptr(out.device)))
    return out


def l2_normalize_rows(x: torch.Tensor, eps: float = _EPS, out: torch.Tensor | None = None) -> torch.Tensor:
    """``x / max(|x|, eps)`` row by row, (rows, dim) fp32.  ``out``: where the rows go instead of a new tensor - float32,
    contiguous, of ``x``'s shape and on its device (``out`` may be ``x`` itself); anything else raises ``MI355Error``."""
    x = _f32c(x, "x")
    if x.dim() != 2:
        raise MI355Error(f"l2_normalize_rows expects (rows, dim), got {tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif not torch.is_tensor(out):
        raise MI355Error(f"l2_normalize_rows: out must be a contiguous float32 tensor, got {type(out).__name__}")
    elif out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device or not out.is_contiguous():
        raise MI355Error(f"l2_normalize_rows: out must be a contiguous float32 {tuple(x.shape)} tensor on {x.device}, got "
                         f"{out.dtype} {tuple(out.shape)} on {out.device}, strides {tuple(out.stride())}")
    with torch.cuda.device(x.device):
        check(lib().mi355_l2_normalize_rows(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], eps,
                                            stream_ptr(x.device)))
    return out


def _check_qg(q, g):
    """Queries against a gallery, a tensor or the ``_Rows`` of a call: both 2-D, the same dim, the same device."""
    if len(q.shape) != 2 or len(g.shape) != 2:
        raise MI355Error(f"expected (Q,D) queries and (G,D) gallery, got {tuple(q.shape)} and {tuple(g.shape)}")
    if q.shape[1] != g.shape[1]:
        raise MI355Error(f"embedding dims differ: {q.shape[1]} vs {g.shape[1]}")
    if q.device != g.device:
        raise MI355Error(f"queries on {q.device} but gallery on {g.device}")


def _row_stride(t: torch.Tensor) -> int:
    """Elements from one row of a 2-D buffer to the next (a single row has no stride of its own: its width)."""
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


class _Rows:
    """The gallery side of a call: the first ``rows`` rows and ``dim`` columns of ``buf`` - fp32 rows, ``normalized`` or not, an
    fp16 gallery buffer (``mi355_gallery_to_f16`` layout: normalised rows, zero padding) or the int8 codes of
    ``mi355_gallery_to_i8`` with their ``scales`` - ``ld`` elements apart.
    ``planes``: the bf16 planes of the same rows (``PreparedGallery``); without ``buf`` they serve the searches they cover."""

    def __init__(self, buf, rows: int, dim: int, normalized: bool, planes: torch.Tensor | None = None,
                 scales: torch.Tensor | None = None):
        self.buf, self.rows, self.dim, self.normalized, self.planes = buf, int(rows), int(dim), bool(normalized), planes
        self.scales = scales
        self.shape = (self.rows, self.dim)
        self.dtype = torch.float32 if buf is None else buf.dtype
        self.device = planes.device if buf is None else buf.device
        self.ld = self.dim if buf is None else _row_stride(buf)

    @classmethod
    def of(cls, gallery, normalized: bool = False) -> "_Rows":
        """``gallery`` if it is resident rows already, else the fp32 rows of a (G, D) device tensor (no copy if it is one)."""
        if isinstance(gallery, cls):
            return gallery
        g = _f32c(gallery, "gallery")
        if g.dim() != 2:
            raise MI355Error(f"expected a (G,D) gallery, got {tuple(g.shape)}")
        return cls(g, g.shape[0], g.shape[1], normalized)

    @property
    def data(self) -> torch.Tensor:
        """The (rows, dim) view of the buffer (fp16: without the row padding)."""
        return self.buf[: self.rows, : self.dim]

    def c_args(self):
        """The gallery arguments every search entry takes after (queries, Q): fp16 and int8 rows are normalised by their
        layout, int8 codes travel with their scales, packed fp4 codes (uint8) with their multipliers."""
        if self.dtype in (torch.int8, torch.uint8):
            return (self.buf.data_ptr(), self.scales.data_ptr(), self.rows, self.dim)
        norm = () if self.dtype == torch.float16 else (int(self.normalized),)
        return (self.buf.data_ptr(), self.rows, self.dim) + norm


# per row dtype, each C entry beside the function that sizes its workspace
_ENTRIES = {
    torch.float32: {"topk": ("mi355_rank_topk", "mi355_rank_topk_filtered", "mi355_rank_workspace_bytes"),
                    "range": ("mi355_cosine_range", "mi355_range_workspace_bytes"),
                    "positives": ("mi355_positives_range", "mi355_range_workspace_bytes"),
                    "ranks": ("mi355_rank_positives", "mi355_rank_positives_workspace_bytes"),
                    "roc": ("mi355_roc_pairs_hist", "mi355_roc_pairs_workspace_bytes")},
    torch.float16: {"topk": ("mi355_rank_topk_f16", "mi355_rank_topk_f16_filtered", "mi355_rank_f16_workspace_bytes"),
                    "range": ("mi355_cosine_range_f16", "mi355_range_f16_workspace_bytes"),
                    "positives": ("mi355_positives_range_f16", "mi355_range_f16_workspace_bytes"),
                    "ranks": ("mi355_rank_positives_f16", "mi355_rank_positives_f16_workspace_bytes"),
                    "roc": ("mi355_roc_pairs_hist_f16", "mi355_roc_pairs_f16_workspace_bytes")},
    # the int8 rows of an Int8Gallery (quantized.py): top-k and range search only
    torch.int8: {"topk": ("mi355_rank_topk_i8", "mi355_rank_topk_i8_filtered", "mi355_rank_i8_workspace_bytes"),
                 "range": ("mi355_cosine_range_i8", "mi355_range_i8_workspace_bytes")},
    # the packed e2m1 rows of an FP4Gallery (fp4.py), two codes per uint8: the same two searches
    torch.uint8: {"topk": ("mi355_rank_topk_fp4", "mi355_rank_topk_fp4_filtered", "mi355_rank_fp4_workspace_bytes"),
                  "range": ("mi355_cosine_range_fp4", "mi355_range_fp4_workspace_bytes")},
}


def cosine_scores(queries: torch.Tensor, gallery: torch.Tensor, eps: float = _EPS,
                  gallery_is_normalized: bool = False) -> torch.Tensor:
    """(Q,D) x (G,D) -> (Q,G) fp32 cosine matrix."""
    q, g = _f32c(queries, "queries"), _f32c(gallery, "gallery")
    _check_qg(q, g)
    Q, D = q.shape
    G = g.shape[0]
    out = torch.empty((Q, G), dtype=torch.float32, device=q.device)
    if Q == 0 or G == 0:
        return out
    nbytes = lib().mi355_rank_workspace_bytes(Q, G, D, 0)
    ws = _ws.get(q.device, nbytes)
    with torch.cuda.device(q.device):
        check(lib().mi355_cosine_scores(q.data_ptr(), Q, g.data_ptr(), G, D, int(gallery_is_normalized), eps,
                                        out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(q.device)))
    return out


_LABEL_MODES = {None: LABEL_ANY, "same": LABEL_SAME, "different": LABEL_DIFFERENT}


def _int64_on(t, name: str, n: int, device) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise MI355Error(f"{name} must be a tensor")
    require_cuda(t, name)
    if t.device != torch.device(device):
        raise MI355Error(f"{name} is on {t.device} but the search runs on {device}")
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise MI355Error(f"{name} must hold integers, got {t.dtype}")
    if t.dim() != 1 or t.shape[0] != n:
        raise MI355Error(f"{name} must have shape ({n},), got {tuple(t.shape)}")
    return t.to(torch.int64).contiguous()


def _need_labels(labels, rows: int, what: str, source: str) -> torch.Tensor:
    """The labels of ``rows`` resident rows for an operation that cannot do without them (``what``; ``source`` says where
    they come from): the one check behind ``Gallery`` and ``ShardedGallery``."""
    if labels is None:
        raise MI355Error(f"{what} needs {source}")
    if labels.shape[0] != rows:
        raise MI355Error(f"{what}: {labels.shape[0]} labels for {rows} rows ({source})")
    return labels


def _rank_filter(Q: int, G: int, device, query_labels, gallery_labels, label_filter, exclude):
    """The mi355_rank_filter of a filtered search, and the int64 tensors it points at (kept alive by the caller), or
    None when no filter argument is given (the unfiltered search runs, exactly as before)."""
    if label_filter not in _LABEL_MODES:
        raise MI355Error(f'label_filter must be None, "same" or "different", got {label_filter!r}')
    if label_filter is None and exclude is None:
        return None
    keep = []
    f = RankFilter()
    f.label_mode = _LABEL_MODES[label_filter]
    if label_filter is not None:
        if query_labels is None or gallery_labels is None:
            raise MI355Error(f'label_filter="{label_filter}" needs query_labels and gallery labels')
        ql = _int64_on(query_labels, "query_labels", Q, device)
        gl = _int64_on(gallery_labels, "gallery_labels", G, device)
        keep += [ql, gl]
        f.query_labels, f.gallery_labels = ql.data_ptr(), gl.data_ptr()
    if exclude is not None:
        ex = _int64_on(exclude, "exclude", Q, device)
        keep.append(ex)
        f.exclude = ex.data_ptr()
    return f, keep


def cosine_topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, eps: float = _EPS,
                gallery_is_normalized: bool = False, idx_offset: int = 0, query_labels: torch.Tensor | None = None,
                gallery_labels: torch.Tensor | None = None, label_filter: str | None = None,
                exclude: torch.Tensor | None = None):
    """All-pairs cosine + top-k: the loop of train/train.py:249-251 as one call.

    Returns (values (Q,k) fp32, indices (Q,k) int64), sorted by descending score; equal scores are
    ordered by ascending gallery index.  Raises like ``torch.topk`` when k exceeds the gallery size.

    Filtered search: ``label_filter="same"`` / ``"different"`` keeps the gallery rows whose label equals / differs from the
    query's (``query_labels`` (Q,), ``gallery_labels`` (G,)); ``exclude`` (Q,) int64 leaves out row ``exclude[q]`` (a global
    index, compared with ``row + idx_offset``; negative = none).  Scores and order are those of the unfiltered search on the
    eligible rows; slots beyond the eligible rows hold (-inf, -1)."""
    return _topk(queries, _Rows.of(gallery, gallery_is_normalized), k, eps, idx_offset, query_labels, gallery_labels,
                 label_filter, exclude)


def _topk(queries: torch.Tensor, rows: _Rows, k: int, eps: float = _EPS, idx_offset: int = 0, query_labels=None,
          gallery_labels=None, label_filter=None, exclude=None):
    """Top-k of ``queries`` against ``rows``, the one search behind ``cosine_topk``, ``PreparedGallery`` and ``Gallery``: an
    unfiltered search that the planes cover (``PreparedGallery.supports``) runs on them, every other one on the fp32 or fp16
    rows (fp16: score = qn . float(row) with fp32 accumulation; order, ties and NaN as ``cosine_topk``)."""
    q = _f32c(queries, "queries")
    _check_qg(q, rows)
    Q, G = q.shape[0], rows.rows
    if k > G or k < 1:
        raise MI355Error(f"selected index k out of range: k={k}, gallery rows={G}")
    filt = _rank_filter(Q, G, q.device, query_labels, gallery_labels, label_filter, exclude)
    vals = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=q.device)
    if Q == 0:
        return vals, idx
    on_planes = filt is None and rows.planes is not None and PreparedGallery.supports(Q, k)
    if not on_planes and rows.buf is None:
        raise MI355Error(f"prepared search needs k <= 8 and more than 4 queries (got k={k}, Q={Q}): use cosine_topk on the rows")
    L = lib()
    plain, filtered, ws_bytes = _ENTRIES[torch.float32 if on_planes else rows.dtype]["topk"]
    ws = _ws.get(q.device, getattr(L, ws_bytes)(Q, G, rows.dim, k))
    out = (vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(q.device))
    with torch.cuda.device(q.device):
        if on_planes:
            check(L.mi355_rank_topk_prepared(q.data_ptr(), Q, rows.planes.data_ptr(), G, rows.dim, k, eps, int(idx_offset), *out))
        elif filt is None:
            check(getattr(L, plain)(q.data_ptr(), Q, *rows.c_args(), k, eps, int(idx_offset), *out))
        else:
            check(getattr(L, filtered)(q.data_ptr(), Q, *rows.c_args(), k, eps, int(idx_offset), filt[0], *out))
    return vals, idx


class PreparedGallery:
    """The three bf16 planes of a gallery's NORMALISED rows in the cosine GEMM's fragment order (6 B per element): made once
    for a resident gallery (``mi355_gallery_prepare``), so that a search does no per-call work on the gallery side - the
    reference re-reads and re-normalises the whole gallery for every query (train/train.py:250)."""

    def __init__(self, gallery_normalized: torch.Tensor):
        g = _f32c(gallery_normalized, "gallery")
        if g.dim() != 2 or g.shape[0] < 1:
            raise MI355Error(f"a prepared gallery needs (G, D) rows with G >= 1, got {tuple(g.shape)}")
        self.rows, self.dim, self.device = int(g.shape[0]), int(g.shape[1]), g.device
        nbytes = lib().mi355_gallery_planes_bytes(self.rows, self.dim)
        self.planes = torch.empty((nbytes,), dtype=torch.uint8, device=g.device)
        with torch.cuda.device(g.device):
            check(lib().mi355_gallery_prepare(g.data_ptr(), self.rows, self.dim, self.planes.data_ptr(), nbytes,
                                              stream_ptr(g.device)))

    @staticmethod
    def supports(Q: int, k: int) -> bool:
        """The prepared path covers the fused selection's range; other shapes use the fp32 rows (``cosine_topk``)."""
        return Q > 4 and 1 <= k <= 8

    def search(self, queries: torch.Tensor, k: int, eps: float = _EPS, idx_offset: int = 0):
        """``cosine_topk(queries, rows, k, gallery_is_normalized=True)`` - same values, indices and argument checks, bit for
        bit - for the shapes ``supports`` covers; any other non-empty query batch raises (the planes alone cannot serve it)."""
        return _topk(queries, _Rows(None, self.rows, self.dim, True, self.planes), k, eps, idx_offset)


def topk(scores: torch.Tensor, k: int, idx_offset: int = 0):
    """``torch.topk(sim, k)`` over the last dim of a 1-D or 2-D fp32 score tensor."""
    squeeze = scores.dim() == 1
    s = _f32c(scores.unsqueeze(0) if squeeze else scores, "scores")
    if s.dim() != 2:
        raise MI355Error(f"topk expects a 1-D or 2-D tensor, got {tuple(scores.shape)}")
    Q, G = s.shape
    if k > G or k < 1:
        raise MI355Error(f"selected index k out of range: k={k}, row length={G}")
    vals = torch.empty((Q, k), dtype=torch.float32, device=s.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=s.device)
    if Q:
        nbytes = lib().mi355_rank_workspace_bytes(Q, G, 0, k)
        ws = _ws.get(s.device, nbytes)
        with torch.cuda.device(s.device):
            check(lib().mi355_topk_rows(s.data_ptr(), Q, G, k, int(idx_offset), vals.data_ptr(), idx.data_ptr(),
                                        ws.data_ptr(), ws.numel(), stream_ptr(s.device)))
    return (vals[0], idx[0]) if squeeze else (vals, idx)


def merge_topk(cand_val: torch.Tensor, cand_idx: torch.Tensor, k: int):
    """Merge (Q, ncand) candidate lists (e.g. all-gathered per-shard top-k) into the global top-k."""
    v = _f32c(cand_val, "cand_val")
    require_cuda(cand_idx, "cand_idx")
    i = cand_idx.to(torch.int64).contiguous()
    if v.shape != i.shape or v.dim() != 2:
        raise MI355Error(f"merge_topk expects matching (Q, ncand) tensors, got {tuple(v.shape)} / {tuple(i.shape)}")
    Q, n = v.shape
    if k > n or k < 1:
        raise MI355Error(f"selected index k out of range: k={k}, candidates={n}")
    vals = torch.empty((Q, k), dtype=torch.float32, device=v.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=v.device)
    if Q:
        nbytes = lib().mi355_rank_workspace_bytes(Q, n, 0, k)
        ws = _ws.get(v.device, nbytes)
        with torch.cuda.device(v.device):
            check(lib().mi355_merge_topk(v.data_ptr(), i.data_ptr(), Q, n, k, vals.data_ptr(), idx.data_ptr(),
                                         ws.data_ptr(), ws.numel(), stream_ptr(v.device)))
    return vals, idx


def pack_candidates(vals: "torch.Tensor | None", idx: "torch.Tensor | None", Q: int, k: int, device) -> torch.Tensor:
    """(Q, kk) local top-k results (kk <= k; None for an empty shard) -> (Q, k, 2) int32 {score bits, LOCAL row index},
    missing slots = {-inf, -1}: the one tensor a rank contributes to the sharded search's candidate all-gather."""
    packed = torch.empty((Q, k, 2), dtype=torch.int32, device=device)
    kk = 0 if vals is None else vals.shape[1]
    if Q:
        v = _f32c(vals, "vals") if kk else None
        i = idx.to(torch.int64).contiguous() if kk else None
        with torch.cuda.device(packed.device):
            check(lib().mi355_pack_candidates(v.data_ptr() if kk else None, i.data_ptr() if kk else None, Q, kk, k,
                                              packed.data_ptr(), stream_ptr(packed.device)))
    return packed


def merge_packed_topk(packed: torch.Tensor, shard_offsets: torch.Tensor, k: int):
    """All-gathered packed candidates (world, Q, k, 2) int32 + the shards' first global rows (world,) int64 on the device
    -> global top-k (values (Q, k) f32, indices (Q, k) int64): offsets, unpacking and the merge run in the library."""
    require_cuda(packed, "packed candidates")
    if packed.dtype != torch.int32 or packed.dim() != 4 or packed.shape[3] != 2 or packed.shape[2] != k:
        raise MI355Error(f"merge_packed_topk expects (world, Q, {k}, 2) int32, got {packed.dtype} {tuple(packed.shape)}")
    packed = packed.contiguous()
    world, Q = packed.shape[0], packed.shape[1]
    off = shard_offsets.to(packed.device, torch.int64).contiguous().view(-1)
    if off.numel() != world:
        raise MI355Error(f"merge_packed_topk: {off.numel()} shard offsets for {world} shards")
    vals = torch.empty((Q, k), dtype=torch.float32, device=packed.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=packed.device)
    if Q:
        ws = _ws.get(packed.device, lib().mi355_merge_packed_workspace_bytes(Q, world, k))
        with torch.cuda.device(packed.device):
            check(lib().mi355_merge_packed_topk(packed.data_ptr(), off.data_ptr(), world, Q, k, vals.data_ptr(),
                                                idx.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(packed.device)))
    return vals, idx


def pair_cosine(a: torch.Tensor, b: torch.Tensor, eps: float = _EPS) -> torch.Tensor:
    """Row-wise cos(a[i], b[i]) — inference/inference.py:226."""
    a, b = _f32c(a, "a"), _f32c(b, "b")
    if a.shape != b.shape or a.dim() != 2:
        raise MI355Error(f"pair_cosine expects two (B,D) tensors, got {tuple(a.shape)} / {tuple(b.shape)}")
    out = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    if a.shape[0]:
        with torch.cuda.device(a.device):
            check(lib().mi355_pair_cosine(a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], eps, out.data_ptr(),
                                          stream_ptr(a.device)))
    return out


class CosineSimilarity(torch.nn.Module):
    """``torch.nn.CosineSimilarity(dim=1, eps)`` for the two call shapes on the hot path:
    (1,D) vs (G,D) -> (G,)   [train/train.py:250]   and   (B,D) vs (B,D) -> (B,)   [inference.py:226]."""

    def __init__(self, dim: int = 1, eps: float = _EPS):
        super().__init__()
        if dim != 1:
            raise MI355Error("only dim=1 (the reference's setting) is implemented")
        self.dim, self.eps = dim, eps

    def forward(self, x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        if x1.dim() != 2 or x2.dim() != 2:
            raise MI355Error(f"CosineSimilarity expects 2-D inputs, got {tuple(x1.shape)} / {tuple(x2.shape)}")
        if x1.shape == x2.shape and x1.shape[0] != 1:
            return pair_cosine(x1, x2, self.eps)
        if x1.shape[0] == 1:
            return cosine_scores(x1, x2, self.eps)[0]
        if x2.shape[0] == 1:
            return cosine_scores(x2, x1, self.eps)[0]
        raise MI355Error(f"unsupported broadcast {tuple(x1.shape)} vs {tuple(x2.shape)}")


class ContrastiveLoss(torch.nn.Module):
    """utils/contrastive_loss.py:6-61, forward only (the inference loop calls it under no_grad,
    inference/inference.py:193-204)."""

    def __init__(self, margin):
        super().__init__()
        self.margin, self.eps = margin, 1e-9

    def forward(self, fm1, fm2, label, mean=True):
        a, b = _f32c(fm1, "fm1"), _f32c(fm2, "fm2")
        if a.shape != b.shape or a.dim() != 2:
            raise MI355Error(f"ContrastiveLoss expects two (B,D) tensors, got {tuple(a.shape)} / {tuple(b.shape)}")
        out = torch.empty((), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            check(lib().mi355_contrastive_loss(a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], float(label),
                                               float(self.margin), int(bool(mean)), out.data_ptr(), None,
                                               stream_ptr(a.device)))
        return out


class CosineEmbeddingLoss(torch.nn.Module):
    """``torch.nn.CosineEmbeddingLoss(margin)`` for the reference's call shape: two (B,D) batches and a scalar
    target of +1 or -1 (``labels["pos"]`` / ``labels["neg"]``, train/train.py:81, :214-216).  Forward only."""

    def __init__(self, margin: float = 0.0, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise MI355Error("reduction must be 'mean' or 'sum'")
        self.margin, self.reduction = margin, reduction

    def forward(self, input1, input2, target):
        a, b = _f32c(input1, "input1"), _f32c(input2, "input2")
        if a.shape != b.shape or a.dim() != 2:
            raise MI355Error(f"CosineEmbeddingLoss expects two (B,D) tensors, got {tuple(a.shape)} / {tuple(b.shape)}")
        t = float(target.reshape(-1)[0].item()) if torch.is_tensor(target) else float(target)
        if torch.is_tensor(target) and target.numel() != 1:
            raise MI355Error("only a scalar (broadcast) target is supported, as in the reference")
        out = torch.empty((), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            check(lib().mi355_cosine_embedding_loss(a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], t,
                                                    float(self.margin), int(self.reduction == "mean"), out.data_ptr(),
                                                    stream_ptr(a.device)))
        return out


def validation_metrics(fm_ims, fm_poss, fm_negs, clss, margin: float = 0.5, k: int = 3):
    """The metric half of ``validation_step`` (train/train.py:308-373) as a handful of batched launches instead of a
    Python loop with one cosine + topk + ``.item()`` per row: cosine-embedding losses (+1 / -1 targets), mean pair
    cosines (``cos_sims`` / ``cos_unsims``), and top-1 / top-3 of every query against the positives of the batch.
    Values stay on the device; nothing here synchronises."""
    cel = CosineEmbeddingLoss(margin)
    loss_pos = cel(fm_ims, fm_poss, 1.0)
    loss_neg = cel(fm_ims, fm_negs, -1.0)
    vals, inds = cosine_topk(fm_ims, fm_poss, min(k, fm_poss.shape[0]))
    counts = hit_counts(inds, clss, clss)
    n = fm_ims.shape[0]
    return {"loss_cos_poss": loss_pos, "loss_cos_negs": loss_neg, "loss_cos": loss_pos + loss_neg,
            "cos_sims": pair_cosine(fm_ims, fm_poss).mean(), "cos_unsims": pair_cosine(fm_ims, fm_negs).mean(),
            "top1": counts[0].float() / n, "top3": counts[1].float() / n, "topk_vals": vals, "topk_inds": inds}


def hit_counts(idx: torch.Tensor, query_cls: torch.Tensor, gallery_cls: torch.Tensor):
    """train/train.py:252-255 -> (top1_hits, top3_hits) as a device int64[2] tensor (no sync)."""
    require_cuda(idx, "idx")
    idx = idx.to(torch.int64).contiguous()
    qc = query_cls.to(idx.device, torch.int64).contiguous()
    gc = gallery_cls.to(idx.device, torch.int64).contiguous()
    if idx.dim() != 2 or qc.shape[0] != idx.shape[0]:
        raise MI355Error("hit_counts expects idx (Q,k) and query_cls (Q,)")
    counts = torch.zeros(2, dtype=torch.int64, device=idx.device)
    if idx.shape[0]:
        with torch.cuda.device(idx.device):
            check(lib().mi355_hit_counts(idx.data_ptr(), idx.shape[0], idx.shape[1], qc.data_ptr(), gc.data_ptr(),
                                         gc.numel(), counts.data_ptr(), stream_ptr(idx.device)))
    return counts


def distinct_class_topn(idx: torch.Tensor, val: torch.Tensor, gallery_cls: torch.Tensor, n: int = 3):
    """Notebook raw :240-251: first n distinct classes along each ranked list."""
    require_cuda(idx, "idx")
    idx = idx.to(torch.int64).contiguous()
    val = _f32c(val, "val")
    gc = gallery_cls.to(idx.device, torch.int64).contiguous()
    Q, k = idx.shape
    oc = torch.empty((Q, n), dtype=torch.int64, device=idx.device)
    oi = torch.empty((Q, n), dtype=torch.int64, device=idx.device)
    ov = torch.empty((Q, n), dtype=torch.float32, device=idx.device)
    if Q:
        with torch.cuda.device(idx.device):
            check(lib().mi355_distinct_class_topn(idx.data_ptr(), val.data_ptr(), Q, k, gc.data_ptr(), gc.numel(), n,
                                                  oc.data_ptr(), oi.data_ptr(), ov.data_ptr(),
                                                  stream_ptr(idx.device)))
    return oc, oi, ov


def _score_boost(score, eps, alpha, threshold, mode):
    s = _f32c(score, "score")
    out = torch.empty_like(s)
    if s.numel():
        with torch.cuda.device(s.device):
            check(lib().mi355_score_boost(s.data_ptr(), s.numel(), float(eps), float(alpha), float(threshold), mode,
                                          out.data_ptr(), stream_ptr(s.device)))
    return out


def cos_sim_score_with_threshold(score: torch.Tensor, eps: float, alpha: float, threshold: float) -> torch.Tensor:
    """utils/score_booster.py:1-20 over a whole fp32 score tensor (the reference takes one score at a time and
    prints it; the print is not reproduced)."""
    return _score_boost(score, eps, alpha, threshold, 0)


def cos_sim_score_booster(score: torch.Tensor, eps: float, alpha: float, mode: str) -> torch.Tensor:
    """utils/score_booster.py:22-37; ``mode`` is "for_pos" or "for_neg" (anything else returns None there; here it raises)."""
    if mode not in ("for_pos", "for_neg"):
        raise MI355Error(f'cos_sim_score_booster: mode must be "for_pos" or "for_neg", got {mode!r}')
    return _score_boost(score, eps, alpha, 0.0, 1 if mode == "for_pos" else 2)


def _gallery_f16_bytes(rows: int, dim: int) -> int:
    return int(lib().mi355_gallery_f16_bytes(rows, dim))


def _f16_stride(dim: int) -> int:
    """Row stride (elements) of an fp16 gallery buffer: ``dim`` rounded up to a multiple of 64 (128 B), padded with zeros."""
    return (int(dim) + 63) // 64 * 64


# ---- alpha query expansion (alpha-QE) and database-side augmentation (DBA): Radenovic, Tolias and Chum, TPAMI 2018
def _qe_args(n, alpha):
    """(n, alpha) checked: n an integer >= 1, alpha a finite float >= 0."""
    if not _is_int(n) or int(n) < 1:
        raise MI355Error(f"query expansion needs n >= 1 neighbours, got {n!r}")
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        raise MI355Error(f"alpha must be a finite float >= 0, got {alpha!r}") from None
    if not np.isfinite(a) or a < 0:
        raise MI355Error(f"alpha must be a finite float >= 0, got {alpha!r}")
    return int(n), a


def _qe_pair(qe):
    if not isinstance(qe, (tuple, list)) or len(qe) != 2:
        raise MI355Error(f"qe must be a pair (n, alpha), got {qe!r}")
    return _qe_args(*qe)


_DTYPES = {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16}


def _expand_rows(base: torch.Tensor, normalize_base: bool, gallery: torch.Tensor, gallery_dtype, G: int, dim: int,
                 vals: torch.Tensor, idx: torch.Tensor, alpha: float, eps: float, idx_offset: int = 0,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """One ``mi355_expand_rows`` launch: row r of ``out`` = normalised (base_r + sum_j w_j * gallery[idx[r, j] - idx_offset]).
    base (R, >= dim) rows (fp32, or the gallery's dtype), gallery (>= G, ld) rows, vals / idx (R, n) of a search; out: (R, dim)
    fp32 (allocated when None) or rows of an fp16 gallery buffer.  Arguments checked by the caller and the library."""
    R, n = vals.shape
    if out is None:
        out = torch.empty((R, dim), dtype=torch.float32, device=base.device)
    if R == 0:
        return out
    vals = vals.contiguous()
    idx = idx.to(torch.int64).contiguous()
    out_dt = _DTYPES[out.dtype]
    ws = _ws.get(base.device, max(int(lib().mi355_expand_workspace_bytes(R, dim, out_dt)), 1))
    with torch.cuda.device(base.device):
        check(lib().mi355_expand_rows(base.data_ptr(), _DTYPES[base.dtype], base.stride(0), int(bool(normalize_base)),
                                      gallery.data_ptr(), _DTYPES[gallery_dtype], int(G), gallery.stride(0), int(dim),
                                      vals.data_ptr(), idx.data_ptr(), R, n, int(idx_offset), float(alpha), float(eps),
                                      out.data_ptr(), out_dt, out.stride(0), ws.data_ptr(), ws.numel(),
                                      stream_ptr(base.device)))
    return out


def expand_queries(queries: torch.Tensor, gallery: torch.Tensor, n: int, alpha: float = 3.0, *,
                   gallery_is_normalized: bool = False, eps: float = _EPS, idx_offset: int = 0,
                   query_labels: torch.Tensor | None = None, gallery_labels: torch.Tensor | None = None,
                   label_filter: str | None = None, exclude: torch.Tensor | None = None) -> torch.Tensor:
    """Alpha query expansion (Radenovic, Tolias and Chum, TPAMI 2018; alpha = 0 is the average QE of Chum et al. 2007).

    Round 1 is ``cosine_topk(queries, gallery, n, ...)`` with the filter arguments as given (slots it leaves empty are
    (-inf, -1)).  Query q then becomes ``l2_normalize_rows(qn + sum_j w_j * row(i_j))``: qn = ``l2_normalize_rows(q)`` (same
    bits), row(i) the gallery's normalised row (``gallery_is_normalized=False`` normalises the gallery once for this), w_j =
    v_j ** alpha for a slot with v_j > 0 and a real row; every other slot is skipped (a NaN row behind it never enters the
    sum).  The sum is fp32 in rank order, the normalisation that of ``l2_normalize_rows`` bit for bit; every row depends
    only on its own query and neighbours (no atomics).  One HIP launch (``mi355_expand_rows``).  Returns (Q, D) fp32."""
    n, alpha = _qe_args(n, alpha)
    q, rows = _f32c(queries, "queries"), _Rows.of(gallery, gallery_is_normalized)
    _check_qg(q, rows)
    Q, D = q.shape
    if Q == 0:
        return torch.empty((0, D), dtype=torch.float32, device=q.device)
    vals, idx = _topk(q, rows, n, eps, idx_offset, query_labels, gallery_labels, label_filter, exclude)
    g = rows.buf if gallery_is_normalized else l2_normalize_rows(rows.buf, eps)
    return _expand_rows(q, True, g, torch.float32, g.shape[0], D, vals, idx, alpha, eps, idx_offset)


def _recall(got_idx: torch.Tensor, want_idx: torch.Tensor, k: int):
    """(mean, per_query (Q,) float64): the share of each row of ``want_idx`` (Q, k) that the same row of ``got_idx`` holds;
    no query: (1.0, empty)."""
    per = (got_idx.unsqueeze(2) == want_idx.unsqueeze(1)).any(dim=1).sum(dim=1).double() / float(k)
    return (float(per.mean()) if per.numel() else 1.0), per


def _filter_from(filt, q0: int):
    """``filt`` (what ``_rank_filter`` returned for a batch of queries) for the queries from ``q0`` on, as ``filter_from`` does
    in C: the same gallery labels and mode, the per-query arrays entered ``q0`` int64 later."""
    if filt is None or not q0:
        return filt
    f, keep = filt
    r = RankFilter(f.query_labels and f.query_labels + 8 * q0, f.gallery_labels, f.label_mode, f.exclude and f.exclude + 8 * q0)
    return r, keep


_MAX_K = 1024                       # the largest k of any search, and the longest shortlist


class _RowStore:
    """What ``Gallery``, ``Int8Gallery`` (quantized.py), ``PQGallery`` (pq.py) and ``BinaryGallery`` (binary.py) share: ``rows``
    labelled rows of ``dim`` columns on ``device``, resident in the buffers a class names in ``_BUFFERS`` (one row each per
    gallery row, all of one capacity), which only grow.  A class says how a block of rows is written (``_write``); growth,
    labels, recall and the rules of a shortlist that ``refine=`` rescores are here."""

    _BUFFERS: tuple = ()

    def __init__(self, dim: int, device, eps: float):
        self.dim, self.device, self.eps = int(dim), torch.device(device), eps
        self.rows, self.labels = 0, None

    def __len__(self):
        return self.rows

    def _reserve(self, n: int) -> None:
        """Room for ``n`` rows: past the capacity every buffer moves to one of ``max(n, 1.5 * capacity + 1024)`` rows."""
        old_cap = getattr(self, self._BUFFERS[0]).shape[0]
        if n > old_cap:
            cap = max(n, int(old_cap * 1.5) + 1024)
            for name in self._BUFFERS:
                old = getattr(self, name)
                new = torch.empty((cap,) + tuple(old.shape[1:]), dtype=old.dtype, device=self.device)
                new[: self.rows].copy_(old[: self.rows])
                _retire(old, self.device)                        # the queued copy still reads the old buffer
                setattr(self, name, new)

    def _add_labels(self, labels) -> None:
        """The labels of a block of rows behind those held so far (int64, on the device); None leaves them as they are."""
        if labels is not None:
            lab = labels.to(self.device, torch.int64)
            if self.labels is not None:
                _retire(self.labels, self.device)
                lab = torch.cat([self.labels, lab])
            self.labels = lab

    def _append(self, e: torch.Tensor, labels, **how):
        """The checked (n, dim) fp32 rows ``e`` behind the resident ones: ``_write(e, first_row, **how)`` fills the buffers."""
        n = e.shape[0]
        self._reserve(self.rows + n)
        if n:
            self._write(e, self.rows, **how)
        self._add_labels(labels)
        self.rows += n
        return self

    def _new_rows(self, embeddings: torch.Tensor) -> torch.Tensor:
        """The argument of ``add`` as contiguous fp32 rows on the GPU, (n, dim)."""
        e = _f32c(embeddings, "embeddings")
        if e.dim() != 2 or e.shape[1] != self.dim:
            raise MI355Error(f"gallery rows must be (n,{self.dim}), got {tuple(e.shape)}")
        return e

    def _labels_for(self, what: str) -> torch.Tensor:
        return _need_labels(self.labels, self.rows, what, "gallery labels: add(embeddings, labels)")

    def _recall_against(self, exact, queries: torch.Tensor, k: int, **search_kwargs):
        """``_recall`` of ``search(queries, k, **search_kwargs)`` against the search of ``exact``, a ``Gallery`` of the same rows."""
        if not isinstance(exact, Gallery) or len(exact) != self.rows:
            raise MI355Error(f"recall needs a Gallery of the same {self.rows} rows")
        got = self.search(queries, k, **search_kwargs)[1]
        return _recall(got, exact.search(queries, k)[1], k)

    def _shortlist_length(self, k, refine, shortlist):
        """(k, R) of a search over these rows: the checked k, and the rows the first scan returns per query - k itself, or with
        ``refine`` the length of the shortlist it rescores.  The one set of rules behind ``PQGallery.search``,
        ``Int8Gallery.search`` and every list index (a store that takes ``refine`` has a ``_NOUN``)."""
        top = min(_MAX_K, self.rows)
        if not _is_int(k) or not 1 <= k <= top:
            raise MI355Error(f"selected index k out of range: k={k!r} outside [1, {top}] (min({_MAX_K}, rows))")
        k = int(k)
        if refine is None:
            if shortlist is not None:
                raise MI355Error("shortlist is the length of the list that refine= rescores: give refine too")
            return k, k
        if not isinstance(refine, Gallery):
            raise MI355Error(f"refine must be a Gallery of the same rows, got {type(refine).__name__}")
        if refine.device != self.device:
            raise MI355Error(f"refine is on {refine.device} but the {self._NOUN} lives on {self.device}")
        if len(refine) != self.rows or refine.dim != self.dim:
            raise MI355Error(f"refine holds {len(refine)} rows of dim {refine.dim}, the {self._NOUN} {self.rows} of dim {self.dim}")
        R = min(max(10 * k, 100), top) if shortlist is None else shortlist
        if not _is_int(R) or not k <= R <= top:
            raise MI355Error(f"shortlist={R!r} outside [k={k}, {top}] (min({_MAX_K}, rows))")
        return k, int(R)

    def _refined_topk(self, q: torch.Tensor, vals: torch.Tensor, idx: torch.Tensor, k: int, refine, idx_offset):
        """The tail of a refined search: the shortlist ``idx`` (Q, R) of the queries ``q`` is scored again against ``refine``'s
        rows (``mi355_rescore_candidates``, into ``vals``), then ``merge_topk`` and ``clear_pads``."""
        Q, R, L, dev = idx.shape[0], idx.shape[1], lib(), self.device
        ws = _ws.get(dev, L.mi355_rescore_candidates_workspace_bytes(Q, self.dim))
        with torch.cuda.device(dev):
            check(L.mi355_rescore_candidates(q.data_ptr(), Q, self.dim, self.eps, refine._buf.data_ptr(), _DTYPES[refine.dtype],
                                             refine._ld, self.rows, idx.data_ptr(), R, int(idx_offset), vals.data_ptr(),
                                             ws.data_ptr(), ws.numel(), stream_ptr(dev)))
        v, i = merge_topk(vals, idx, k)
        clear_pads(v, i, int(idx_offset), int(idx_offset) + self.rows)
        return v, i


class _GraphIndexed:
    """``Gallery.graph``: the cached ``GraphIndex`` (graph.py) of a gallery's rows.  It lives in a base of ``Gallery`` because
    the index, like the PQ classes, is exported lazily and carries its own side-stream cases (tests/test_graph_gpu.py covers
    ``Gallery.graph``) instead of a row in the stream table, which lists what ``Gallery`` itself defines."""

    def graph(self, nentry: int, degree: int = 32, **kw):
        """The ``GraphIndex`` of the resident rows with ``nentry`` entry points: ``GraphIndex.build(self, nentry,
        degree=degree, **kw)`` (``iters``, ``seed``, ``init``).  Cached per (nentry, degree, iters, seed) until ``add``; an index
        built from a given ``init`` is not cached."""
        from . import graph as _graph
        if kw.get("init") is not None:
            return _graph.GraphIndex.build(self, nentry, degree=degree, **kw)
        key = (nentry, degree, kw.get("iters", 10), kw.get("seed", 0))
        if key not in self._graph:
            self._graph[key] = _graph.GraphIndex.build(self, nentry, degree=degree, **kw)
        return self._graph[key]


class _DensityClustered:
    """``Gallery.dbscan`` and ``Gallery.components`` (cluster.py).  They live in a base of ``Gallery`` for the reason
    ``_GraphIndexed`` does: their side-stream case is tests/test_dbscan_streams_gpu.py, not a row of the stream table, which
    lists what ``Gallery`` itself defines."""

    def dbscan(self, threshold: float, min_samples: int = 5, **kw):
        """``dbscan`` of the resident rows (fp32 or fp16, read where they lie): a ``DBSCANResult`` whose hits are those of
        ``range_search(self.data.float(), threshold)``.  Keywords as there (``block``).  Not cached."""
        from . import cluster as _cl
        return _cl.dbscan(self, threshold, min_samples, eps=self.eps, **kw)

    def components(self, threshold: float, **kw):
        """``connected_components`` of the resident rows' threshold graph: ``dbscan(threshold, 1)``.  Not cached."""
        from . import cluster as _cl
        return _cl.connected_components(self, threshold, eps=self.eps, **kw)


class _Diffused:
    """``Gallery.diffusion_index`` and ``Gallery.diffuse`` (diffusion.py).  They live in a base of ``Gallery`` for the reason
    ``_GraphIndexed`` does: ``DiffusionIndex`` is exported lazily and the side-stream case is
    tests/test_diffusion_streams_gpu.py, not a row of the stream table, which lists what ``Gallery`` itself defines."""

    def diffusion_index(self, kd: int = 20, gamma: int = 3):
        """The ``DiffusionIndex`` of the resident rows for (kd, gamma): the kNN graph and the symmetric normalised affinity rows
        of its mutual edges (``nbytes`` tells its size).  Cached until ``add``."""
        from . import diffusion as _df
        key = _df.index_params(self.rows, kd, gamma)
        if key not in self._diffusion:
            self._diffusion[key] = _df.DiffusionIndex(self, *key)
        return self._diffusion[key]

    def diffuse(self, queries: torch.Tensor, k: int, *, kd: int = 20, kq: int = 10, alpha: float = 0.99, gamma: int = 3,
                iters: int = 20, shortlist: int | None = None, exclude: torch.Tensor | None = None, idx_offset: int = 0,
                stats: bool = False):
        """Diffusion re-ranking (Iscen et al., CVPR 2017; truncated to the shortlist, see diffusion.py): ``search(queries,
        shortlist)``, then ``(I - alpha S_L) f = y`` by at most ``iters`` conjugate-gradient iterations on the part of the
        gallery's mutual kNN graph (``kd`` neighbours, affinity ``max(score, 0)^gamma``) inside the shortlist, ``y`` the
        affinities of the first ``kq`` shortlist rows.  Returns the top-k of the shortlist by descending f as (values (Q, k) fp32,
        indices (Q, k) int64), ties to the earlier shortlist position, pads (-inf, -1) last; with ``stats=True`` also the
        iterations done per query (Q,) int32.  ``shortlist``: k <= shortlist <= min(rows, 1024), default min(rows, max(k, 200));
        1 <= kq <= shortlist; alpha in (0, 1); gamma in [1, 8]; iters in [1, 64]; ``exclude`` / ``idx_offset`` as in ``search``."""
        from . import diffusion as _df
        return _df.diffuse(self, queries, k, kd=kd, kq=kq, alpha=alpha, gamma=gamma, iters=iters, shortlist=shortlist,
                           exclude=exclude, idx_offset=idx_offset, stats=stats)


class _Diversified:
    """``Gallery.diversify`` (diversify.py).  It lives in a base of ``Gallery`` for the reason ``_Diffused`` does: ``mmr_rerank``
    is exported lazily and the side-stream case is tests/test_diversify_streams_gpu.py, not a row of the stream table, which lists
    what ``Gallery`` itself defines."""

    def diversify(self, queries: torch.Tensor, k: int, *, lam: float = 0.7, dedup=None, shortlist: int | None = None,
                  exclude: torch.Tensor | None = None, idx_offset: int = 0, stats: bool = False, block: int | None = None):
        """The k best *different* results (maximal marginal relevance, Carbonell and Goldstein 1998; see diversify.py):
        ``search(queries, shortlist)``, the Gram matrix S of each shortlist's rows (their fp16 values on the f16 MFMA), then k
        greedy picks: the eligible slot of greatest ``lam * score - (1 - lam) * m``, ``m`` the slot's largest S against the picks
        so far, ties to the earlier slot.  With ``dedup=t`` a slot is ineligible once ``m >= t`` (near-duplicate suppression;
        ``lam=1, dedup=t`` walks the plain order and keeps a row unless it is within t of a kept one).  Returns, in pick order,
        (the picks' cosine scores (Q, k) fp32 - not monotone -, indices (Q, k) int64); when the eligible slots run out the rest is
        (-inf, -1).  ``stats=True`` adds the MMR values at pick time (Q, k) fp32 and the picks per query (Q,) int32.
        ``shortlist``: k <= shortlist <= min(rows, 1024), default min(rows, max(10 k, 100), 1024); lam in [0, 1]; ``block``: queries
        whose Gram matrices are held at once (default: what fits 256 MiB; results do not depend on it); ``exclude`` / ``idx_offset``
        as in ``search``.  ``lam=1`` without ``dedup`` is ``search(queries, shortlist)[:, :k]``."""
        from . import diversify as _dv
        return _dv.diversify(self, queries, k, lam=lam, dedup=dedup, shortlist=shortlist, exclude=exclude, idx_offset=idx_offset,
                             stats=stats, block=block)


class _ScoreNormed:
    """``Gallery.score_norm``, ``Gallery.search_normed`` and ``Gallery.neighbourhood_stats`` (scorenorm.py).  They live in a base of
    ``Gallery`` for the reason ``_Diversified`` does: the module's names are exported lazily and the side-stream case is
    tests/test_scorenorm_streams_gpu.py, not a row of the stream table, which lists what ``Gallery`` itself defines."""

    def neighbourhood_stats(self, cohort, n: int | None = None, exclude: torch.Tensor | None = None):
        """(mean, std, count) of each resident row's ``n`` largest cosines against ``cohort`` (a (C, D) tensor or a ``Gallery``;
        ``n=None``: the whole cohort, at most 1024 rows): float64 sums, the population deviation.  ``exclude`` (rows,) int64 leaves
        one cohort row out per resident row, for a cohort that contains the rows themselves."""
        from . import scorenorm as _sn
        return _sn.neighbourhood_stats(self.data, cohort, n, exclude=exclude, eps=self.eps)

    def score_norm(self, cohort, kind: str = "csls", n: int | None = None, min_std: float = 1e-6):
        """A ``ScoreNorm`` of this gallery (scorenorm.py): ``kind="csls"`` removes hubs (``cohort``: samples of the query domain;
        n = 10), "znorm" / "tnorm" / "snorm" centre and scale a pair's score by each side's scores against an impostor ``cohort``
        (``n=None``: the whole cohort; a given n: the adaptive variant).  Fit again after ``add``."""
        from . import scorenorm as _sn
        return _sn.ScoreNorm.fit(self, cohort, kind, n, min_std)

    def search_normed(self, queries: torch.Tensor, k: int, norm, idx_offset: int = 0, *, query_labels: torch.Tensor | None = None,
                      label_filter: str | None = None, exclude: torch.Tensor | None = None):
        """``search`` over the scores that ``norm`` (``score_norm``) adjusts: (adjusted values (Q, k) fp32, indices (Q, k) int64),
        descending, ties to the lower index; the filter arguments as in ``search``.  The adjustment runs inside the cosine GEMM in
        front of the fused selection; a prepared gallery is searched on its fp32 rows (same results)."""
        from . import scorenorm as _sn
        if not isinstance(norm, _sn.ScoreNorm):
            raise MI355Error(f"norm must be a ScoreNorm (Gallery.score_norm), got {type(norm).__name__}")
        return norm.search(self, queries, k, idx_offset, query_labels=query_labels, label_filter=label_filter, exclude=exclude)


class Gallery(_RowStore, _GraphIndexed, _DensityClustered, _Diffused, _Diversified, _ScoreNormed):
    """Resident gallery: rows are L2-normalised once when added and stay in HBM (the gallery is *born* on the
    GPU that embedded it).  ``search`` is then one fused call per query batch instead of the reference's per-query cosine +
    topk pair.

    ``dtype=torch.float32`` (default) keeps the normalised rows as fp32.  ``dtype=torch.float16`` keeps
    ``fp16(l2_normalize_rows(x))`` - bit for bit ``l2_normalize_rows(x).half()``, not renormalised after rounding - in a
    buffer whose rows are padded with zeros to a multiple of 64 elements: half the bytes of fp32 rows.  Its search scores
    ``qn . float(row)`` (``qn`` normalised as in ``cosine_topk``) with fp32 accumulation, |error| ~1e-7, and orders results as
    ``cosine_topk`` does (descending, ties to the lower index, NaN first)."""

    def __init__(self, dim: int, device, capacity: int = 0, eps: float = _EPS, dtype: torch.dtype = torch.float32):
        if dtype not in (torch.float32, torch.float16):
            raise MI355Error(f"Gallery dtype must be torch.float32 or torch.float16, got {dtype}")
        super().__init__(dim, device, eps)
        self.dtype = dtype
        if dtype == torch.float16 and self.dim < 1:
            raise MI355Error(f"an fp16 Gallery needs dim >= 1, got {dim}")
        self._ld = _f16_stride(self.dim) if dtype == torch.float16 else self.dim
        self._buf = torch.empty((max(capacity, 0), self._ld), dtype=dtype, device=self.device)
        self._prepared, self._prepared_rows = None, 0
        self._knn, self._rerank = {}, {}                         # per k1 / (k1, k2); dropped by add
        self._ivf = {}                                           # per (nlist, iters, seed); dropped by add
        self._graph = {}                                         # per (nentry, degree, iters, seed); dropped by add
        self._diffusion = {}                                     # per (kd, gamma); dropped by add

    _BUFFERS = ("_buf",)

    def _write(self, e: torch.Tensor, r0: int) -> None:
        n = e.shape[0]
        out = self._buf[r0: r0 + n]
        if self.dtype == torch.float16:
            with torch.cuda.device(e.device):
                check(lib().mi355_gallery_to_f16(e.data_ptr(), n, self.dim, 0, self.eps, out.data_ptr(),
                                                 _gallery_f16_bytes(n, self.dim), stream_ptr(e.device)))
        else:
            l2_normalize_rows(e, self.eps, out=out)

    def add(self, embeddings: torch.Tensor, labels: torch.Tensor | None = None):
        self._append(self._new_rows(embeddings), labels)
        self._knn, self._rerank = {}, {}
        self._ivf = {}
        self._graph = {}
        self._diffusion = {}
        return self

    @property
    def data(self) -> torch.Tensor:
        """The (rows, dim) normalised rows (a view; for fp16 without the row padding)."""
        return self._resident().data

    def _resident(self) -> _Rows:
        """The rows as the gallery side of a call, with the planes of ``prepare()`` while no row was added since."""
        fresh = self._prepared is not None and self._prepared_rows == self.rows
        return _Rows(self._buf, self.rows, self.dim, True, self._prepared.planes if fresh else None)

    @property
    def nbytes(self) -> int:
        """Resident footprint in bytes: the row buffer at its current capacity, plus the bf16 planes of ``prepare()``."""
        p = self._prepared
        return self._buf.numel() * self._buf.element_size() + (p.planes.numel() if p is not None else 0)

    def prepare(self):
        """Split the resident rows once into the GEMM's bf16 planes (PreparedGallery, +6 B per element): searches with k <= 8
        and more than 4 queries then run without touching the fp32 rows.  Call again after ``add``.  fp32 galleries only."""
        if self.dtype != torch.float32:
            raise MI355Error("prepare() makes bf16 planes of fp32 rows; an fp16 gallery is searched as it is")
        self._prepared = PreparedGallery(self.data) if self.rows else None
        self._prepared_rows = self.rows
        return self

    def quantized(self):
        """An ``Int8Gallery`` (quantized.py) of the resident rows of an fp32 gallery: the rows are normalised already, so its
        codes and scales are bit for bit those of ``Int8Gallery.add`` of the original embeddings.  Labels are copied."""
        from .quantized import Int8Gallery
        if self.dtype != torch.float32:
            raise MI355Error("quantized() makes int8 codes of fp32 rows; quantise the embeddings with Int8Gallery.add instead")
        out = Int8Gallery(self.dim, self.device, capacity=self.rows, eps=self.eps)
        out._append(self.data, None if self.labels is None else self.labels.clone(), normalized=True)
        return out

    def search(self, queries: torch.Tensor, k: int, idx_offset: int = 0, *, query_labels: torch.Tensor | None = None,
               label_filter: str | None = None, exclude: torch.Tensor | None = None, qe=None):
        """Top-k of ``queries`` against the resident rows.  ``label_filter`` ("same" / "different") compares the gallery's
        labels (``add(..., labels)``) with ``query_labels``; ``exclude`` leaves out one global row per query (see
        ``cosine_topk``).  A filtered search on a prepared gallery runs on its fp32 rows (same results).

        ``qe=(n, alpha)``: alpha query expansion - exactly ``search(expand_queries(queries, n, alpha, ...), k, ...)``, the same
        filter arguments in both rounds (so a leave-one-out search never expands a query with its own row)."""
        if qe is not None:
            n, alpha = _qe_pair(qe)
            filt = dict(query_labels=query_labels, label_filter=label_filter, exclude=exclude)
            return self.search(self.expand_queries(queries, n, alpha, idx_offset, **filt), k, idx_offset, **filt)
        gl = None if label_filter is None else self._labels_for(f'label_filter="{label_filter}"')
        return _topk(queries, self._resident(), k, self.eps, idx_offset, query_labels, gl, label_filter, exclude)

    def expand_queries(self, queries: torch.Tensor, n: int, alpha: float = 3.0, idx_offset: int = 0, *,
                       query_labels: torch.Tensor | None = None, label_filter: str | None = None,
                       exclude: torch.Tensor | None = None) -> torch.Tensor:
        """Alpha query expansion against the resident rows: ``search(queries, n, ...)`` (whichever path ``search`` takes,
        filters as given), then each query becomes ``l2_normalize_rows(qn + sum_j v_j^alpha * row(i_j))`` over its used slots
        (score > 0, a real row), summed in fp32 in rank order (fp16 rows widened exactly) by one HIP launch
        (``mi355_expand_rows``).  Returns (Q, dim) fp32."""
        n, alpha = _qe_args(n, alpha)
        q = _f32c(queries, "queries")
        _check_qg(q, self._resident())
        if q.shape[0] == 0:
            return torch.empty((0, self.dim), dtype=torch.float32, device=q.device)
        vals, idx = self.search(q, n, idx_offset, query_labels=query_labels, label_filter=label_filter, exclude=exclude)
        return _expand_rows(q, True, self._buf, self.dtype, self.rows, self.dim, vals, idx, alpha, self.eps, idx_offset)

    def augmented(self, n: int, alpha: float = 3.0, block: int = 256) -> "Gallery":
        """Database-side augmentation: a NEW gallery (same dtype, dim, eps and labels; unprepared) whose row r is
        ``l2_normalize_rows(row_r + sum_j v_j^alpha * row(i_j))`` over the top-n of row r against this gallery with row r
        itself left out (``exclude=arange``), every sum taken from the ORIGINAL rows; fp16 rows are stored as ``add`` would
        store that fp32 row.  The self-join runs ``block`` rows at a time through ``search``, each block followed by one
        expansion launch.  This gallery is not changed."""
        n, alpha = _qe_args(n, alpha)
        G = self.rows
        out = Gallery(self.dim, self.device, capacity=G, eps=self.eps, dtype=self.dtype)
        out.labels = None if self.labels is None else self.labels.clone()
        if G == 0:
            return out
        if n > G:
            raise MI355Error(f"selected index k out of range: k={n}, gallery rows={G}")
        block = max(int(block), 1)
        for q0 in range(0, G, block):
            qn = min(block, G - q0)
            ex = torch.arange(q0, q0 + qn, dtype=torch.int64, device=self.device)
            vals, idx = self.search(self.data[q0: q0 + qn], n, exclude=ex)
            _expand_rows(self._buf[q0: q0 + qn], False, self._buf, self.dtype, G, self.dim, vals, idx, alpha, self.eps, 0,
                         out=out._buf[q0: q0 + qn])
        out.rows = G
        return out

    def knn_graph(self, k1: int, block: int = 256):
        """The kNN graph of the resident rows: (vals (rows, k1) fp32, idx (rows, k1) int64), the top-k1 OTHER rows of every row
        and their scores, as ``search(row, k1, exclude=row)`` orders them (a prepared gallery: on its fp32 rows).  The
        self-join runs ``block`` rows per search, as ``augmented`` does.  1 <= k1 <= 32, k1 < rows.  Cached per k1 until ``add``."""
        from . import rerank as _rr
        k1, _ = _rr.graph_params(self.rows, k1)
        if k1 not in self._knn:
            self._knn[k1] = _rr.knn_graph(self, k1, block)
        return self._knn[k1]

    def rerank_index(self, k1: int = 20, k2: int = 6):
        """The ``RerankIndex`` of the resident rows for (k1, k2): the kNN graph, tau and the sparse rows V and V' of every
        gallery row (``nbytes`` tells its size).  Cached until ``add``."""
        from . import rerank as _rr
        key = _rr.graph_params(self.rows, k1, k2)
        if key not in self._rerank:
            self._rerank[key] = _rr.RerankIndex(self, *key)
        return self._rerank[key]

    def rerank(self, queries: torch.Tensor, k: int, *, k1: int = 20, k2: int = 6, lam: float = 0.3,
               shortlist: int | None = None, exclude: torch.Tensor | None = None, idx_offset: int = 0):
        """k-reciprocal re-ranking (Zhong et al., CVPR 2017; gallery-graph variant, see rerank.py): ``search(queries, shortlist)``
        re-scored as s* = 1 - ((1 - lam) dJ + lam (1 - s)), dJ the Jaccard distance of the sparse k-reciprocal vectors of the
        query and the row; returns the top-k of the shortlist by descending s* as (values (Q, k) fp32, indices (Q, k) int64),
        ties to the earlier shortlist position, pads (-inf, -1) last.  ``shortlist``: k <= shortlist <= min(rows, 1024), default
        min(rows, max(k, 100)); ``exclude`` / ``idx_offset`` as in ``search``.  ``lam=1`` is the plain search order."""
        from . import rerank as _rr
        return _rr.rerank(self, queries, k, k1=k1, k2=k2, lam=lam, shortlist=shortlist, exclude=exclude, idx_offset=idx_offset)

    def moments(self):
        """``embedding_moments`` of the resident normalised rows (fp32 or fp16, read where they lie): the input of a PCA
        whitening fit (``Whitening.fit(gallery)``)."""
        from .whitening import embedding_moments
        return embedding_moments(self)

    def whitened(self, w, dtype: torch.dtype | None = None) -> "Gallery":
        """A NEW gallery of ``w.dim_out`` columns (same eps and labels, unprepared; ``dtype`` as this one unless given) whose
        row r is the whitening ``w`` of resident row r - the rows are normalised already, so they go into the projection as
        they are - written straight into the new buffer by one ``mi355_whiten_rows`` launch (fp16: rounded as ``add`` would
        store that fp32 row).  Query side: ``whitened.search(w.transform(q), k)``.  This gallery is not changed."""
        if self.dim != w.dim_in:
            raise MI355Error(f"the whitening takes {w.dim_in} columns but the gallery has {self.dim}")
        out = Gallery(w.dim_out, self.device, capacity=self.rows, eps=self.eps, dtype=self.dtype if dtype is None else dtype)
        out.labels = None if self.labels is None else self.labels.clone()
        w._apply(self._resident(), False, out._buf[: self.rows], True)
        out.rows = self.rows
        return out

    def range_search(self, queries: torch.Tensor, threshold: float, *, query_labels: torch.Tensor | None = None,
                     label_filter: str | None = None, exclude: torch.Tensor | None = None, max_results: int | None = None,
                     idx_offset: int = 0) -> RangeResult:
        """``cosine_range`` of ``queries`` against the resident rows: every row whose score is >= ``threshold``, with the
        scores of this gallery's own kernel (fp32 rows: ``cosine_scores`` of the normalised rows, a prepared gallery
        included; fp16 rows: the f16-MFMA kernel).  ``label_filter`` uses the labels given to ``add``."""
        gl = None if label_filter is None else self._labels_for(f'label_filter="{label_filter}"')
        return _range(queries, self._resident(), threshold, self.eps, idx_offset, query_labels, gl, label_filter, exclude,
                      max_results)

    def verification_roc(self, queries: torch.Tensor, query_labels: torch.Tensor, thresholds=None,
                         exclude: torch.Tensor | None = None):
        """``verification_roc`` of ``queries`` against the resident rows and the labels given to ``add``.  Each pair's score
        has the bits of this gallery's own search (fp32 rows: ``cosine_scores`` of its normalised rows; fp16 rows: the
        f16-MFMA kernel)."""
        gl = self._labels_for("verification_roc")
        require_cuda(queries, "queries")
        thr = _roc_thresholds(thresholds, self.device)
        return _roc_finalize(_roc_hist(queries, query_labels, self._resident(), gl, exclude, 0, thr, self.eps), thr)


    def ranking_metrics(self, queries: torch.Tensor, query_labels: torch.Tensor, *, exclude: torch.Tensor | None = None,
                        ranks=(1, 5, 10, 20)):
        """``ranking_metrics`` of ``queries`` against the resident rows and the labels given to ``add``: full-gallery mAP and
        CMC, every score with the bits of this gallery's own search (fp32 or fp16 rows; the planes of ``prepare()`` are not
        used).  ``exclude`` (Q,) leaves out one global row per query (negative: none)."""
        gl = self._labels_for("ranking_metrics")
        rows = self._resident()
        _ranking_args(queries, query_labels, rows, gl)
        return _ranking_metrics(queries, query_labels, rows, gl, exclude, 0, _cmc_ranks(ranks), self.eps)

    def kmeans(self, n_clusters: int, **kw):
        """``spherical_kmeans`` of the resident rows (fp32 or fp16, read where they lie): a ``KMeansResult``.  Keywords as
        there (``iters``, ``seed``, ``init``, ``block``)."""
        from . import cluster as _cl
        return _cl.spherical_kmeans(self, n_clusters, eps=self.eps, **kw)

    def ivf(self, nlist: int, **kw):
        """The ``IVFIndex`` of the resident rows with ``nlist`` lists: ``IVFIndex.build(self, nlist, **kw)`` (``iters``,
        ``seed``, ``init``).  Cached per (nlist, iters, seed) until ``add``; an index built from a given ``init`` is not cached."""
        from . import ivf as _ivf
        if kw.get("init") is not None:
            return _ivf.IVFIndex.build(self, nlist, **kw)
        key = (nlist, kw.get("iters", 10), kw.get("seed", 0))
        if key not in self._ivf:
            self._ivf[key] = _ivf.IVFIndex.build(self, nlist, **kw)
        return self._ivf[key]

    def clustering_metrics(self, n_clusters: int | None = None, **kw) -> dict:
        """Clusters the resident rows (``kmeans``; ``n_clusters`` defaults to the number of distinct labels given to ``add``)
        and scores the clusters against those labels: ``clustering_metrics(kmeans(K).assignments, labels)`` - NMI, purity and
        pairwise F1."""
        from . import cluster as _cl
        gl = self._labels_for("clustering_metrics")
        if n_clusters is None:
            n_clusters = int(torch.unique(gl).shape[0])
        return _cl.clustering_metrics(self.kmeans(n_clusters, **kw).assignments, gl)


def clear_pads(vals: torch.Tensor, idx: torch.Tensor, lo: int, hi: int):
    """In place: entries whose index lies outside [lo, hi) become (-inf, -1)."""
    require_cuda(idx, "idx")
    if vals.dtype != torch.float32 or idx.dtype != torch.int64 or not vals.is_contiguous() or not idx.is_contiguous():
        raise MI355Error("clear_pads expects contiguous fp32 values and int64 indices")
    if vals.numel():
        with torch.cuda.device(idx.device):
            check(lib().mi355_clear_pads(vals.data_ptr(), idx.data_ptr(), idx.numel(), int(lo), int(hi), stream_ptr(idx.device)))
    return vals, idx


_MAX_R = 1024


def retrieval_accuracy(queries: torch.Tensor, query_labels: torch.Tensor, gallery: torch.Tensor | None = None,
                       gallery_labels: torch.Tensor | None = None, ks=(1, 2, 4, 8), eps: float = _EPS,
                       query_expansion=None):
    """Leave-one-out / cross-source retrieval accuracy of labelled embeddings, as defined by Musgrave et al. 2020 ("A Metric
    Learning Reality Check") and pytorch-metric-learning's AccuracyCalculator.

    ``gallery=None``: the queries are their own gallery and every query's own row is excluded (one ``cosine_topk`` with
    ``exclude=arange(Q)``).  Otherwise ``gallery`` (G, D) with ``gallery_labels`` (G,).  R_q = the number of gallery rows
    with the query's label (its own row not counted); queries with R_q = 0 are left out of every mean (``num_lone``).  One
    search with k = max(max(ks), max R_q) (at most 1024) ranks every query; the per-query metrics run in one HIP kernel
    (``mi355_retrieval_metrics``); classes above 1024 rows: ``ranking_metrics`` ranks every positive.  Returns device tensors (float64) ``precision_at_1``, ``recall_at_k`` {K: ...},
    ``r_precision``, ``map_at_r``, and ints ``num_queries``, ``num_lone``.  The one host sync reads max R_q.

    ``query_expansion=(n, alpha)``: the queries are first replaced by ``expand_queries(queries, gallery, n, alpha)`` with the
    same exclusion (same-source: a query is never expanded with its own row), then ranked as above."""
    q = _f32c(queries, "queries")
    if q.dim() != 2:
        raise MI355Error(f"queries must be (Q, D), got {tuple(q.shape)}")
    Q = q.shape[0]
    ql = _int64_on(query_labels, "query_labels", Q, q.device)
    same_source = gallery is None
    if same_source:
        if gallery_labels is not None:
            raise MI355Error("gallery_labels given without a gallery (same-source evaluation uses query_labels)")
        g, gl = q, ql
    else:
        g = _f32c(gallery, "gallery")
        _check_qg(q, g)
        if gallery_labels is None:
            raise MI355Error("a gallery needs gallery_labels")
        gl = _int64_on(gallery_labels, "gallery_labels", g.shape[0], q.device)
    G = g.shape[0]
    ks = sorted({int(K) for K in ks})
    if not ks or ks[0] < 1 or ks[-1] > _MAX_R:
        raise MI355Error(f"ks must be ranks in [1, {_MAX_R}], got {ks}")
    if Q == 0 or G == 0 or (same_source and G < 2):
        raise MI355Error(f"retrieval_accuracy needs queries and at least one other gallery row (Q={Q}, G={G})")
    # class sizes in the gallery -> R_q
    if same_source:
        _, inv, counts = torch.unique(ql, return_inverse=True, return_counts=True)
        R = counts[inv] - 1
    else:
        uniq, inv = torch.unique(torch.cat([gl, ql]), return_inverse=True)
        R = torch.bincount(inv[:G], minlength=uniq.numel())[inv[G:]]
    r_max = int(R.max().item())                                # the one host sync
    if r_max > _MAX_R:
        lab = int(ql[int(R.argmax().item())].item())
        raise MI355Error(f"class {lab} has {r_max} relevant gallery rows; retrieval_accuracy ranks at most {_MAX_R}")
    k = min(max(ks[-1], r_max), G)        # k = G ranks every row, so recall@K for K > G is exact as well
    exclude = torch.arange(Q, dtype=torch.int64, device=q.device) if same_source else None
    if query_expansion is not None:
        n_qe, alpha = _qe_pair(query_expansion)
        q = expand_queries(q, g, n_qe, alpha, eps=eps, exclude=exclude)
    _, idx = cosine_topk(q, g, k, eps, exclude=exclude)
    per = torch.empty((Q, 3), dtype=torch.float64, device=q.device)
    Rc = R.contiguous()
    with torch.cuda.device(q.device):
        check(lib().mi355_retrieval_metrics(idx.data_ptr(), Q, k, ql.data_ptr(), gl.data_ptr(), G, Rc.data_ptr(),
                                            per.data_ptr(), stream_ptr(q.device)))
    valid = (Rc > 0).to(torch.float64)
    n = valid.sum()
    first = per[:, 0]

    def mean(x):
        return (x * valid).sum() / n

    return {"precision_at_1": mean((first == 0).to(torch.float64)),
            "recall_at_k": {K: mean((first < K).to(torch.float64)) for K in ks},
            "r_precision": mean(per[:, 1]), "map_at_r": mean(per[:, 2]),
            "num_queries": Q, "num_lone": (Rc <= 0).sum(), "per_query": per, "R": Rc, "indices": idx}


def retrieval_metrics(queries, positives, query_cls, gallery_cls=None, k: int = 3):
    """The rank loop of inference/inference.py:223-245 with the pinned semantics of train/train.py:
    mean pair cosine, top-1 and top-3 accuracy of ``queries`` against the ``positives`` gallery."""
    gallery_cls = query_cls if gallery_cls is None else gallery_cls
    vals, idx = cosine_topk(queries, positives, k)
    counts = hit_counts(idx, query_cls, gallery_cls)
    pos = pair_cosine(queries, positives) if queries.shape == positives.shape else None
    n = queries.shape[0]
    return {"top1": counts[0].item() / n, "top3": counts[1].item() / n,
            "scores": None if pos is None else pos.mean().item(), "topk_vals": vals, "topk_inds": idx}


# ---- verification ROC (utils/roc_curve_from_scratch.py)
_ROC_MAX_T = 4096


def _roc_thresholds(thresholds, device):
    """(host float64 tensor, the same values on ``device``): the reference's grid ``arange(0, 105, 5) / 100`` by default."""
    if thresholds is None:
        host = torch.from_numpy(np.array(list(range(0, 105, 5))) / 100)
    elif torch.is_tensor(thresholds):
        host = thresholds.detach().to("cpu", torch.float64)
    else:
        host = torch.from_numpy(np.array(thresholds, dtype=np.float64))
    if host.dim() != 1 or not 1 <= host.shape[0] <= _ROC_MAX_T:
        raise MI355Error(f"thresholds must be a 1-D sequence of 1..{_ROC_MAX_T} values, got shape {tuple(host.shape)}")
    if not bool(torch.isfinite(host).all()):
        raise MI355Error("thresholds must be finite")
    if host.shape[0] > 1 and bool((host[1:] < host[:-1]).any()):
        raise MI355Error("thresholds must be ascending")
    host = host.contiguous()
    if torch.device(device).type != "cuda":       # (an injected CPU backend of ShardedGallery)
        return host, host.clone()
    return host, host.pin_memory().to(device, non_blocking=True)


def _dptr(host: torch.Tensor):
    return ctypes.cast(host.data_ptr(), ctypes.POINTER(ctypes.c_double))


def _roc_finalize(hist: torch.Tensor, thr):
    """hist (2, T + 1) int64 -> the result dict of ``roc_curve`` / ``verification_roc`` (one launch: mi355_roc_finalize)."""
    host, dev = thr
    T = host.shape[0]
    counts = torch.empty((4, T), dtype=torch.int64, device=hist.device)
    totals = torch.empty(2, dtype=torch.int64, device=hist.device)
    rates = torch.empty((2, T), dtype=torch.float64, device=hist.device)
    auc = torch.empty((), dtype=torch.float64, device=hist.device)
    with torch.cuda.device(hist.device):
        check(lib().mi355_roc_finalize(hist.data_ptr(), T, counts.data_ptr(), totals.data_ptr(), rates.data_ptr(), auc.data_ptr(),
                                       stream_ptr(hist.device)))
    return {"thresholds": dev, "tp": counts[0], "fp": counts[1], "fn": counts[2], "tn": counts[3], "tpr": rates[0],
            "fpr": rates[1], "auc": auc, "num_genuine": totals[0], "num_impostor": totals[1]}


def roc_curve(scores: torch.Tensor, actual: torch.Tensor, thresholds=None):
    """``roc_curve`` of utils/roc_curve_from_scratch.py on given pair scores, without the plot.

    ``scores`` (n,) fp32 or fp64 and ``actual`` (n,) (1 = genuine, 0 = impostor; any other value is counted in neither class,
    as the reference's if/elif chain does) on the GPU.  A pair is predicted positive at t iff ``score >= t`` in float64
    (pandas' comparison; exact for fp32 scores too).  ``thresholds``: ascending, finite, 1..4096 values (default: the
    reference's 21 points 0, 0.05, .., 1).  Returns device tensors: ``thresholds`` (T,) float64, ``tp``, ``fp``, ``fn``, ``tn``
    (T,) int64, ``tpr``, ``fpr`` (T,) float64 (NaN where a class is empty), ``auc`` = |trapezoid(tpr, fpr)| unrounded (the
    reference prints it rounded to 4 digits), ``num_genuine``, ``num_impostor``."""
    for t, name in ((scores, "scores"), (actual, "actual")):
        if not torch.is_tensor(t):
            raise MI355Error(f"{name} must be a tensor")
        require_cuda(t, name)
    if scores.dtype not in (torch.float32, torch.float64):
        raise MI355Error(f"scores must be float32 or float64, got {scores.dtype}")
    if scores.dim() != 1 or actual.dim() != 1 or actual.shape[0] != scores.shape[0]:
        raise MI355Error(f"scores and actual must be 1-D of the same length, got {tuple(scores.shape)} and {tuple(actual.shape)}")
    if actual.device != scores.device:
        raise MI355Error(f"actual is on {actual.device} but scores on {scores.device}")
    s = scores.contiguous()
    if actual.dtype == torch.bool:
        code = actual.contiguous().view(torch.int8)
    elif actual.dtype == torch.int8:
        code = actual.contiguous()
    else:                                       # 1 -> genuine, 0 -> impostor, everything else (2, 0.5, NaN, 257, ..) -> -1
        code = torch.where(actual == 1, 1, torch.where(actual == 0, 0, -1)).to(torch.int8)
    thr = _roc_thresholds(thresholds, s.device)
    T = thr[0].shape[0]
    hist = torch.empty((2, T + 1), dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        check(lib().mi355_roc_scores_hist(s.data_ptr(), int(s.dtype == torch.float64), s.shape[0], code.data_ptr(), _dptr(thr[0]),
                                          thr[1].data_ptr(), T, hist.data_ptr(), stream_ptr(s.device)))
    return _roc_finalize(hist, thr)


def _roc_hist(queries: torch.Tensor, query_labels, rows: _Rows, gallery_labels, exclude, idx_offset: int, thr,
              eps: float = _EPS) -> torch.Tensor:
    """The (2, T + 1) int64 pair histogram of ``queries`` and their labels against ``rows`` and theirs (row j is global row
    ``j + idx_offset`` for ``exclude``): the one entry behind ``verification_roc``, ``Gallery`` and ``ShardedGallery``."""
    q = _f32c(queries, "queries")
    _check_qg(q, rows)
    Q, G = q.shape[0], rows.rows
    ql = _int64_on(query_labels, "query_labels", Q, q.device)
    gl = _int64_on(gallery_labels, "gallery_labels", G, q.device)
    ex = None if exclude is None else _int64_on(exclude, "exclude", Q, q.device)
    host, dev = thr
    T = host.shape[0]
    if Q == 0 or G == 0:
        return torch.zeros((2, T + 1), dtype=torch.int64, device=q.device)
    hist = torch.empty((2, T + 1), dtype=torch.int64, device=q.device)        # (zeroed by the call)
    L = lib()
    entry, ws_bytes = _ENTRIES[rows.dtype]["roc"]
    ws = _ws.get(q.device, getattr(L, ws_bytes)(Q, G, rows.dim))
    with torch.cuda.device(q.device):
        check(getattr(L, entry)(q.data_ptr(), Q, *rows.c_args(), eps, ql.data_ptr(), gl.data_ptr(), ex.data_ptr() if ex is not None else None,
                                int(idx_offset), _dptr(host), dev.data_ptr(), T, hist.data_ptr(), ws.data_ptr(), ws.numel(),
                                stream_ptr(q.device)))
    return hist


def verification_roc(queries: torch.Tensor, query_labels: torch.Tensor, gallery: torch.Tensor | None = None,
                     gallery_labels: torch.Tensor | None = None, thresholds=None, eps: float = _EPS,
                     exclude: torch.Tensor | None = None, idx_offset: int = 0):
    """Verification ROC over EVERY labelled (query, gallery row) pair: genuine iff the labels are equal, impostor otherwise.

    Each pair's score has the bits ``cosine_scores(queries, gallery)`` gives it (the same GEMM path; Q <= 4 as well), and is
    binned inside the GEMM's epilogue: no (Q, G) score matrix is made.  ``gallery=None``: the queries are their own gallery
    and every ordered pair (i, j), i != j, counts once.  ``exclude`` (Q,) leaves out the pair (q, exclude[q] - idx_offset) (a
    global row, as in ``cosine_topk``; negative = none).  Thresholds and the result as ``roc_curve``; counts are exact
    integers, the same every run."""
    q = _f32c(queries, "queries")
    if q.dim() != 2:
        raise MI355Error(f"queries must be (Q, D), got {tuple(q.shape)}")
    if gallery is None:
        if gallery_labels is not None:
            raise MI355Error("gallery_labels given without a gallery (same-source evaluation uses query_labels)")
        if exclude is not None or idx_offset:
            raise MI355Error("same-source evaluation (gallery=None) excludes each query's own row itself: no exclude / idx_offset")
        gallery, gallery_labels = q, query_labels
        exclude = torch.arange(q.shape[0], dtype=torch.int64, device=q.device)
    elif gallery_labels is None:
        raise MI355Error("a gallery needs gallery_labels")
    thr = _roc_thresholds(thresholds, q.device)
    return _roc_finalize(_roc_hist(q, query_labels, _Rows.of(gallery), gallery_labels, exclude, idx_offset, thr, eps), thr)


# ---- cosine range search: every gallery row at or above a threshold
class RangeResult(NamedTuple):
    """CSR result of ``cosine_range``: the hits of query q are ``indices[offsets[q]:offsets[q + 1]]`` (global rows, ascending)
    with their ``scores``."""
    offsets: torch.Tensor          # (Q + 1,) int64
    indices: torch.Tensor          # (nnz,) int64
    scores: torch.Tensor           # (nnz,) fp32


_cand = _Workspace()               # the search's candidate buffers ([2][capacity] 8-byte entries), grown to the largest need
_MIN_CAPACITY = 1 << 16


def _range_threshold(threshold) -> float:
    t = float(threshold)
    if not np.isfinite(t):
        raise MI355Error(f"threshold must be finite, got {threshold!r}")
    return t


def _range_empty(Q: int, device) -> RangeResult:
    return RangeResult(torch.zeros(Q + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int64, device=device),
                       torch.empty(0, dtype=torch.float32, device=device))


def _range(queries: torch.Tensor, rows: _Rows, threshold: float, eps: float = _EPS, idx_offset: int = 0, query_labels=None,
           gallery_labels=None, label_filter=None, exclude=None, max_results: int | None = None,
           keep_all: bool = False) -> RangeResult:
    """The range search of ``queries`` against ``rows``, the one entry behind ``cosine_range``, ``Gallery`` and
    ``ShardedGallery`` (the planes of a prepared gallery are not used).  One search into the cached candidate buffer; if its
    hits do not fit, ONE more search with exactly that capacity; then the compaction into exact-size outputs.
    ``keep_all`` (``positive_ranks`` only, with ``label_filter="same"``): no threshold, every row the filter keeps is a hit,
    a NaN score included."""
    q = _f32c(queries, "queries")
    _check_qg(q, rows)
    threshold = _range_threshold(threshold)
    Q, G = q.shape[0], rows.rows
    filt = _rank_filter(Q, G, q.device, query_labels, gallery_labels, label_filter, exclude)
    if max_results is not None and int(max_results) < 0:
        raise MI355Error(f"max_results must be >= 0 or None, got {max_results}")
    if Q == 0 or G == 0:
        return _range_empty(Q, q.device)
    L = lib()
    entry, ws_bytes = _ENTRIES[rows.dtype]["positives" if keep_all else "range"]
    ws = _ws.get(q.device, getattr(L, ws_bytes)(Q, G, rows.dim))
    fp = ctypes.byref(filt[0]) if filt is not None else None
    nnz = ctypes.c_int64(0)
    thr = () if keep_all else (threshold,)

    def search(cand):
        cap = cand.numel() // 16
        with torch.cuda.device(q.device):
            check(getattr(L, entry)(q.data_ptr(), Q, *rows.c_args(), eps, *thr, int(idx_offset), fp, cand.data_ptr(), cap,
                                    ctypes.byref(nnz), ws.data_ptr(), ws.numel(), stream_ptr(q.device)))
        return cap, int(nnz.value)

    cand = _cand.get(q.device, 16 * _MIN_CAPACITY)
    cap, n = search(cand)
    if max_results is not None and n > int(max_results):
        raise MI355Error(f"the range search has {n} hits, more than max_results={int(max_results)}")
    if n > cap:                                    # the exact count is known: one more search that fits
        cand = _cand.get(q.device, 16 * n)
        cap, n2 = search(cand)
        if n2 != n:
            raise MI355Error(f"the range search counted {n} hits, then {n2}")
    offsets = torch.empty(Q + 1, dtype=torch.int64, device=q.device)
    indices = torch.empty(n, dtype=torch.int64, device=q.device)
    scores = torch.empty(n, dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        check(L.mi355_range_compact(cand.data_ptr(), cap, Q, n, int(idx_offset), ws.data_ptr(), ws.numel(), offsets.data_ptr(),
                                    indices.data_ptr() if n else None, scores.data_ptr() if n else None, stream_ptr(q.device)))
    return RangeResult(offsets, indices, scores)


def cosine_range(queries: torch.Tensor, gallery: torch.Tensor, threshold: float, *, eps: float = _EPS,
                 gallery_is_normalized: bool = False, idx_offset: int = 0, query_labels: torch.Tensor | None = None,
                 gallery_labels: torch.Tensor | None = None, label_filter: str | None = None,
                 exclude: torch.Tensor | None = None, max_results: int | None = None) -> RangeResult:
    """Every (query, gallery row) pair whose cosine score is ``>= threshold``, as a CSR ``RangeResult(offsets, indices,
    scores)``.

    The comparison is the float64 ``score >= threshold`` of the reference's verification decision (an fp32 score against the
    smallest float not below ``threshold``; a NaN score never qualifies).  Each score has the bits ``cosine_scores`` gives
    the pair on the same path (any Q: the tiled GEMM), and no (Q, G) score matrix is made.  Within a query the rows ascend;
    the result is the same bit for bit on every run.  Filters as in ``cosine_topk`` (``label_filter``, ``exclude``,
    ``idx_offset``).  ``max_results``: raise ``MI355Error`` if there are more hits, before any output is allocated.  One host
    sync per query block (its hit count), as ``torch.nonzero``."""
    return _range(queries, _Rows.of(gallery, gallery_is_normalized), threshold, eps, idx_offset, query_labels, gallery_labels,
                  label_filter, exclude, max_results)


# ---- full-gallery ranks of every positive: mean average precision and the CMC curve (Zheng et al., ICCV 2015)
class PositiveRanks(NamedTuple):
    """CSR result of ``positive_ranks``: the positives of query q are ``indices[offsets[q]:offsets[q + 1]]`` (global rows) in
    rank order, with their ``scores`` and their 1-based ``ranks`` among the query's eligible rows."""
    offsets: torch.Tensor          # (Q + 1,) int64
    indices: torch.Tensor          # (nnz,) int64
    scores: torch.Tensor           # (nnz,) fp32
    ranks: torch.Tensor            # (nnz,) int64


_MAX_G_RANKS = (1 << 31) - 128
_SIGN64 = -(1 << 63)


def _cmc_ranks(ranks):
    """The CMC ranks as a sorted list of distinct positive ints."""
    try:
        rs = list(ranks)
    except TypeError:
        raise MI355Error(f"ranks must be a sequence of positive integers, got {ranks!r}") from None
    if not rs or any(not _is_int(r) or int(r) < 1 for r in rs):
        raise MI355Error(f"ranks must be a non-empty sequence of positive integers, got {ranks!r}")
    return sorted({int(r) for r in rs})


def _ranking_args(queries, query_labels, gallery, gallery_labels):
    """The shape and device checks of ``positive_ranks`` / ``ranking_metrics``, before anything is asked of a device.
    ``gallery``: None (same-source), a (G, D) tensor or the ``_Rows`` of a resident gallery."""
    for t, name in ((queries, "queries"), (query_labels, "query_labels")):
        if not torch.is_tensor(t):
            raise MI355Error(f"{name} must be a tensor")
    if queries.dim() != 2:
        raise MI355Error(f"queries must be (Q, D), got {tuple(queries.shape)}")
    Q = queries.shape[0]
    if gallery is None:
        if gallery_labels is not None:
            raise MI355Error("gallery_labels given without a gallery (same-source evaluation uses query_labels)")
        G = Q
    else:
        if gallery_labels is None:
            raise MI355Error("a gallery needs gallery_labels")
        if not torch.is_tensor(gallery_labels):
            raise MI355Error("gallery_labels must be a tensor")
        _check_qg(queries, gallery)
        G = gallery.shape[0]
        if gallery_labels.dim() != 1 or gallery_labels.shape[0] != G:
            raise MI355Error(f"gallery_labels must have shape ({G},), got {tuple(gallery_labels.shape)}")
    if query_labels.dim() != 1 or query_labels.shape[0] != Q:
        raise MI355Error(f"query_labels must have shape ({Q},), got {tuple(query_labels.shape)}")
    if Q == 0 or G == 0 or (gallery is None and G < 2):
        raise MI355Error(f"ranking needs queries and at least one other gallery row (Q={Q}, G={G})")
    if G >= _MAX_G_RANKS:
        raise MI355Error(f"ranking counts in 32 bits: G={G} must be below {_MAX_G_RANKS}")


def _ranks_positives(q, ql, rows: _Rows, gl, ex, idx_offset, eps):
    """``ranks/positives``: (offsets, keys, indices, scores) of every query's positives in rank order.  The range pass without
    a threshold under ``label_filter="same"`` yields them with the bits of the GEMM; their composites
    (``mi355_rank_positives_keys``) are put into rank order per query by two stable ``torch.sort`` calls (composite descending
    as UNSIGNED 64-bit - the sign bit flipped for the signed sort - then query)."""
    pos = _range(q, rows, 0.0, eps, idx_offset, ql, gl, "same", ex, keep_all=True)
    n, dev = pos.indices.shape[0], q.device
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib().mi355_rank_positives_keys(pos.indices.data_ptr() if n else None, pos.scores.data_ptr() if n else None, n,
                                              int(idx_offset), keys.data_ptr() if n else None, stream_ptr(dev)))
    seg = torch.repeat_interleave(torch.arange(q.shape[0], device=dev), pos.offsets[1:] - pos.offsets[:-1], output_size=n)
    o1 = torch.sort(torch.bitwise_xor(keys, _SIGN64), descending=True, stable=True).indices
    perm = o1[torch.sort(seg[o1], stable=True).indices]
    return pos.offsets, keys[perm].contiguous(), pos.indices[perm].contiguous(), pos.scores[perm].contiguous()


def _ranks_count(q, ql, rows: _Rows, gl, ex, idx_offset, eps, offsets, keys, block=None) -> torch.Tensor:
    """``ranks/count``: before (nnz,) int32, the eligible non-positive rows of each query per bin of positives that beat them
    (``mi355_rank_positives``, the GEMM with the counting epilogue).  The offsets are checked on the host first (one sync)."""
    Q, n, dev = q.shape[0], keys.shape[0], q.device
    before = torch.empty(n, dtype=torch.int32, device=dev)                    # (zeroed by the call)
    off_host = offsets.cpu()
    L = lib()
    entry, ws_bytes = _ENTRIES[rows.dtype]["ranks"]
    ws = _ws.get(dev, getattr(L, ws_bytes)(Q, rows.rows, rows.dim))
    with torch.cuda.device(dev):
        check(getattr(L, entry)(q.data_ptr(), Q, *rows.c_args(), eps, ql.data_ptr(), gl.data_ptr(),
                                ex.data_ptr() if ex is not None else None, int(idx_offset), offsets.data_ptr(),
                                ctypes.cast(off_host.data_ptr(), ctypes.POINTER(ctypes.c_int64)), keys.data_ptr() if n else None, n,
                                before.data_ptr() if n else None, 0 if block is None else int(block), ws.data_ptr(), ws.numel(),
                                stream_ptr(dev)))
    return before


def _ranks_finalize(offsets, before):
    """``ranks/finalize``: (ranks (nnz,) int64, AP (Q,) float64, first rank (Q,) int64) in one launch."""
    Q, n, dev = offsets.shape[0] - 1, before.shape[0], offsets.device
    ranks = torch.empty(n, dtype=torch.int64, device=dev)
    ap = torch.empty(Q, dtype=torch.float64, device=dev)
    first = torch.empty(Q, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib().mi355_rank_positives_finalize(offsets.data_ptr(), before.data_ptr() if n else None, Q, n,
                                                  ranks.data_ptr() if n else None, ap.data_ptr(), first.data_ptr(), stream_ptr(dev)))
    return ranks, ap, first


def _positive_ranks(queries: torch.Tensor, query_labels, rows: _Rows, gallery_labels, exclude=None, idx_offset: int = 0,
                    eps: float = _EPS, block: int | None = None):
    """(``PositiveRanks``, AP (Q,) float64, first rank (Q,) int64) of ``queries`` against ``rows`` (arguments checked by
    ``_ranking_args``): the one entry behind ``positive_ranks``, ``ranking_metrics`` and ``Gallery.ranking_metrics``, in the
    three phases above.  ``block``: queries per GEMM call of the counting pass (for tests; the result does not depend on it).
    Host syncs: the hit count of the range pass and the offsets."""
    q = _f32c(queries, "queries")
    Q, G, dev = q.shape[0], rows.rows, q.device
    ql = _int64_on(query_labels, "query_labels", Q, dev)
    gl = _int64_on(gallery_labels, "gallery_labels", G, dev)
    ex = None if exclude is None else _int64_on(exclude, "exclude", Q, dev)
    if block is not None and int(block) < 1:
        raise MI355Error(f"block must be >= 1, got {block}")
    offsets, keys, indices, scores = _ranks_positives(q, ql, rows, gl, ex, idx_offset, eps)
    before = _ranks_count(q, ql, rows, gl, ex, idx_offset, eps, offsets, keys, block)
    ranks, ap, first = _ranks_finalize(offsets, before)
    return PositiveRanks(offsets, indices, scores, ranks), ap, first


def _same_source(queries, exclude, idx_offset):
    if exclude is not None or idx_offset:
        raise MI355Error("same-source evaluation (gallery=None) excludes each query's own row itself: no exclude / idx_offset")
    return torch.arange(queries.shape[0], dtype=torch.int64, device=queries.device)


def positive_ranks(queries: torch.Tensor, query_labels: torch.Tensor, gallery: torch.Tensor | None = None,
                   gallery_labels: torch.Tensor | None = None, *, eps: float = _EPS, exclude: torch.Tensor | None = None,
                   idx_offset: int = 0, gallery_is_normalized: bool = False) -> PositiveRanks:
    """The rank of every positive of every query in the WHOLE gallery, as a CSR ``PositiveRanks(offsets, indices, scores,
    ranks)`` with each query's positives in rank order.

    Eligible rows of query q: every gallery row except ``exclude[q]`` (a global row, compared with ``row + idx_offset``;
    negative = none); ``gallery=None``: the queries are their own gallery and each query's own row is excluded (its
    duplicates are not).  Positives: eligible rows with the query's label.  The order is ``cosine_topk``'s: descending score,
    NaN first, -0 equal to +0, equal scores to the lower row; every score has the bits ``cosine_scores`` gives the pair on the
    same path (the tiled GEMM for any Q).  ``ranks`` (int64, 1-based) counts the eligible rows up to and including the
    positive.  Neither a (Q, G) score matrix nor a sorted gallery is made: each negative is counted inside the GEMM's epilogue
    into the bin of the positives that beat it.  Integer counts: the same every run."""
    _ranking_args(queries, query_labels, gallery, gallery_labels)
    if gallery is None:
        exclude = _same_source(queries, exclude, idx_offset)
    q = _f32c(queries, "queries")
    if gallery is None:
        gallery, gallery_labels = q, query_labels
    return _positive_ranks(q, query_labels, _Rows.of(gallery, gallery_is_normalized), gallery_labels, exclude, idx_offset, eps)[0]


def _ranking_metrics(queries, query_labels, rows: _Rows, gallery_labels, exclude, idx_offset, ranks, eps):
    pr, ap, first = _positive_ranks(queries, query_labels, rows, gallery_labels, exclude, idx_offset, eps)
    R = pr.offsets[1:] - pr.offsets[:-1]
    valid = (R > 0).to(torch.float64)
    n = valid.sum()

    def mean(x):
        return (x.to(torch.float64) * valid).sum() / n

    return {"map": mean(ap), "cmc": {r: mean((first <= r) & (R > 0)) for r in ranks}, "mean_first_rank": mean(first),
            "per_query_ap": ap, "first_rank": first, "R": R, "num_queries": int(R.shape[0]), "num_lone": (R <= 0).sum(),
            "positive_ranks": pr}


def ranking_metrics(queries: torch.Tensor, query_labels: torch.Tensor, gallery: torch.Tensor | None = None,
                    gallery_labels: torch.Tensor | None = None, *, ranks=(1, 5, 10, 20), eps: float = _EPS,
                    query_expansion=None):
    """Full-gallery mean average precision and the CMC curve of labelled embeddings (the protocol of Zheng et al., ICCV
    2015, that Zhong et al. 2017 report): every positive of every query is ranked among ALL eligible gallery rows
    (``positive_ranks``), whatever the class sizes - ``retrieval_accuracy`` stops at classes of 1024.

    ``gallery=None``: the queries are their own gallery, each query's own row excluded; otherwise ``gallery`` (G, D) with
    ``gallery_labels`` (G,).  With the positives p_0, p_1, .. of query q in rank order and R_q their number:
    AP_q = (sum_i (i + 1) / rank(p_i)) / R_q in float64, the terms added in that order; first_rank_q = rank(p_0); CMC(r) = the
    share of queries with first_rank_q <= r.  Queries with R_q = 0 are left out of every mean and counted in ``num_lone``
    (their ``per_query_ap`` and ``first_rank`` are 0).  Ties, NaN and -0 as ``positive_ranks``.  Returns device tensors
    ``map``, ``cmc`` {r: ...}, ``mean_first_rank`` (float64), ``per_query_ap`` (Q,) float64, ``first_rank`` (Q,) int64, ``R``
    (Q,) int64, ``num_lone``, the int ``num_queries`` and the ``positive_ranks`` themselves.

    ``query_expansion=(n, alpha)``: the queries are first replaced by ``expand_queries(queries, gallery, n, alpha)`` with the
    same exclusion (same-source: a query is never expanded with its own row), then ranked as above."""
    _ranking_args(queries, query_labels, gallery, gallery_labels)
    ranks = _cmc_ranks(ranks)
    q = _f32c(queries, "queries")
    exclude = None
    if gallery is None:
        exclude = _same_source(q, None, 0)
        gallery, gallery_labels = q, query_labels
    g = _f32c(gallery, "gallery")
    if query_expansion is not None:
        n_qe, alpha = _qe_pair(query_expansion)
        q = expand_queries(q, g, n_qe, alpha, eps=eps, exclude=exclude)
    return _ranking_metrics(q, query_labels, _Rows.of(g), gallery_labels, exclude, 0, ranks, eps)
