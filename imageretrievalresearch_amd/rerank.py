"""k-reciprocal re-ranking of search results (Zhong, Zheng, Cao and Li, CVPR 2017; not in the reference), gallery-graph variant.

The neighbourhoods of gallery rows are taken inside the gallery, once per gallery (``Gallery.knn_graph``, a self-join through
``search(..., exclude=arange)``), and kept with their sparse vectors in a ``RerankIndex``; queries are attached to that graph.
Three deviations from the paper's public code: the distance is the fixed ``1 - cos`` (not squared Euclidean divided by a
data-dependent column maximum), the sparse vectors have no query column, and only a shortlist of candidates is re-scored.
No (Q + G)^2 matrix exists at any point: the work after the kNN lists is four HIP entries on CSR rows (csrc/rerank.hip,
definitions in include/mi355_retrieval.h):

* ``_kr_sets`` ....... the expanded reciprocal sets R*(r)         (mi355_kr_sets: count pass, one host sync, fill pass)
* ``_kr_weights`` .... V(r)[j] = exp(-d(r, j)) / sum              (mi355_kr_weights: the gather-dot)
* ``_kr_local_qe`` ... V'(r) = mean of V over the first k2 of N   (mi355_kr_local_qe: count pass, one host sync, fill pass)
* ``_kr_score`` ...... s* = 1 - ((1 - lam) dJ + lam (1 - s))      (mi355_kr_score), then the library's ``topk``

These staged wrappers take and return device tensors, so a test can feed each step fixed discrete inputs."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from ._lib import DTYPE_F16, DTYPE_F32, MI355Error, check, lib, require_cuda, stream_ptr
from .rank import _EPS, Gallery, _check_qg, _f32c, _int64_on, _is_int, l2_normalize_rows, topk

MAX_K1 = 32          # MI355_KR_MAX_K1
MAX_SHORTLIST = 1024
_DT = {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16}


class Csr(NamedTuple):
    """Sparse rows: ``offsets`` (rows + 1,) int64, ``cols`` (nnz,) int32 ascending within a row, ``vals`` (nnz,) fp32."""
    offsets: torch.Tensor
    cols: torch.Tensor
    vals: torch.Tensor

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self)


def _int_in(name: str, v, lo: int, hi: int) -> int:
    if not _is_int(v) or not lo <= int(v) <= hi:
        raise MI355Error(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def graph_params(G: int, k1, k2=1):
    """(k1, k2) checked against a gallery of G rows: 1 <= k1 <= 32, k1 < G, 1 <= k2 <= k1 + 1."""
    k1 = _int_in("k1", k1, 1, MAX_K1)
    if k1 >= G:
        raise MI355Error(f"k1={k1} needs a gallery of more than k1 rows, got {G}")
    return k1, _int_in("k2", k2, 1, k1 + 1)


def rerank_params(G: int, k, k1=20, k2=6, lam=0.3, shortlist=None):
    """(k, k1, k2, lam, K) checked: ``graph_params``, lam a finite float in [0, 1], k >= 1 and the shortlist
    k <= K <= min(G, 1024) (default min(G, max(k, 100)))."""
    k1, k2 = graph_params(G, k1, k2)
    try:
        lam = float(lam)
    except (TypeError, ValueError):
        raise MI355Error(f"lam must be a float in [0, 1], got {lam!r}") from None
    if not np.isfinite(lam) or not 0.0 <= lam <= 1.0:
        raise MI355Error(f"lam must be a finite float in [0, 1], got {lam!r}")
    if not _is_int(k) or int(k) < 1:
        raise MI355Error(f"selected index k out of range: k={k!r}, gallery rows={G}")
    k = int(k)
    top = min(G, MAX_SHORTLIST)
    K = min(G, max(k, 100)) if shortlist is None else shortlist
    if not _is_int(K) or not k <= int(K) <= top:
        raise MI355Error(f"shortlist must be an integer with k={k} <= shortlist <= min(gallery rows, {MAX_SHORTLIST}) = {top}, "
                         f"got {K!r}")
    return k, k1, k2, lam, int(K)


def _lists(t: torch.Tensor, name: str, k1: int | None = None) -> torch.Tensor:
    require_cuda(t, name)
    if t.dim() != 2 or t.dtype != torch.int64 or (k1 is not None and t.shape[1] != k1):
        raise MI355Error(f"{name} must be (rows, {'k1' if k1 is None else k1}) int64, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _nnz(offsets: torch.Tensor) -> int:
    return int(offsets[-1].item())                              # the host sync between a count pass and its fill pass


def _kr_sets(lists: torch.Tensor, graph: torch.Tensor, list_vals: torch.Tensor | None = None, tau: torch.Tensor | None = None):
    """R*(r) of every row of ``lists`` (R, k1) against ``graph`` (G, k1): gallery rows (``lists is graph``, no ``list_vals``) or
    query rows with their scores ``list_vals`` (R, k1) and the gallery's ``tau`` (G,).  Returns (offsets, cols)."""
    graph = _lists(graph, "graph")
    G, k1 = graph.shape
    lists = _lists(lists, "lists", k1)
    R = lists.shape[0]
    dev = graph.device
    if (list_vals is None) != (tau is None):
        raise MI355Error("query rows need both list_vals and tau")
    if list_vals is not None:
        list_vals, tau = _f32c(list_vals, "list_vals"), _f32c(tau, "tau")
        if list_vals.shape != lists.shape or tau.shape != (G,):
            raise MI355Error(f"list_vals must be {tuple(lists.shape)} and tau ({G},), got {tuple(list_vals.shape)} / {tuple(tau.shape)}")
    offsets = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    cols = torch.empty(0, dtype=torch.int32, device=dev)
    if R == 0:
        return offsets, cols
    lv = None if list_vals is None else list_vals.data_ptr()
    tp = None if tau is None else tau.data_ptr()
    with torch.cuda.device(dev):
        check(lib().mi355_kr_sets(lists.data_ptr(), lv, tp, R, k1, graph.data_ptr(), G, offsets.data_ptr(), None, 0,
                                  stream_ptr(dev)))
        nnz = _nnz(offsets)
        if nnz:
            cols = torch.empty(nnz, dtype=torch.int32, device=dev)
            check(lib().mi355_kr_sets(lists.data_ptr(), lv, tp, R, k1, graph.data_ptr(), G, offsets.data_ptr(), cols.data_ptr(),
                                      nnz, stream_ptr(dev)))
    return offsets, cols


def _kr_weights(rows: torch.Tensor, R: int, gallery: torch.Tensor, G: int, dim: int, offsets: torch.Tensor,
                cols: torch.Tensor) -> torch.Tensor:
    """V(r)[j] for the CSR pattern (offsets, cols): the first ``R`` rows of ``rows`` against the first ``G`` rows of ``gallery``
    (2-D fp32 or fp16 buffers of normalised rows, ``dim`` columns used).  Returns vals (nnz,) fp32."""
    for t, name in ((rows, "rows"), (gallery, "gallery"), (offsets, "offsets"), (cols, "cols")):
        require_cuda(t, name)
    if rows.dtype not in _DT or gallery.dtype not in _DT or rows.dim() != 2 or gallery.dim() != 2:
        raise MI355Error(f"rows and gallery must be 2-D fp32 or fp16, got {rows.dtype} {tuple(rows.shape)} / {gallery.dtype} "
                         f"{tuple(gallery.shape)}")
    if rows.shape[0] < R or gallery.shape[0] < G or rows.shape[1] < dim or gallery.shape[1] < dim:
        raise MI355Error(f"embedding dims differ or rows missing: rows {tuple(rows.shape)}, gallery {tuple(gallery.shape)}, "
                         f"R={R}, G={G}, dim={dim}")
    if rows.stride(1) != 1 or gallery.stride(1) != 1 or offsets.dtype != torch.int64 or cols.dtype != torch.int32 \
            or offsets.shape != (R + 1,):
        raise MI355Error("kr_weights expects row-major buffers, int64 offsets (R + 1,) and int32 cols")
    nnz = cols.numel()
    vals = torch.empty(nnz, dtype=torch.float32, device=cols.device)
    if R and nnz:
        with torch.cuda.device(cols.device):
            check(lib().mi355_kr_weights(rows.data_ptr(), _DT[rows.dtype], max(rows.stride(0), dim), R, gallery.data_ptr(),
                                         _DT[gallery.dtype], G, max(gallery.stride(0), dim), dim, offsets.data_ptr(),
                                         cols.data_ptr(), nnz, vals.data_ptr(), stream_ptr(cols.device)))
    return vals


def _kr_local_qe(lists: torch.Tensor, k2: int, own: Csr, gallery: Csr, G: int) -> Csr:
    """V'(r) = (1 / k2) (own row r + gallery rows lists[r][: k2 - 1]); for gallery rows ``own is gallery``."""
    lists = _lists(lists, "lists")
    R, k1 = lists.shape
    dev = lists.device
    offsets = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    empty = Csr(offsets, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev))
    if R == 0:
        return empty
    if own.offsets.shape != (R + 1,) or gallery.offsets.shape != (G + 1,):
        raise MI355Error(f"kr_local_qe: offsets of {own.offsets.shape[0] - 1} own and {gallery.offsets.shape[0] - 1} gallery rows "
                         f"for R={R}, G={G}")
    args = (lists.data_ptr(), R, k1, int(k2), own.offsets.data_ptr(), own.cols.data_ptr() or None, own.vals.data_ptr() or None,
            own.cols.numel(), gallery.offsets.data_ptr(), gallery.cols.data_ptr() or None, gallery.vals.data_ptr() or None,
            gallery.cols.numel(), G, offsets.data_ptr())
    with torch.cuda.device(dev):
        check(lib().mi355_kr_local_qe(*args, None, None, 0, stream_ptr(dev)))
        nnz = _nnz(offsets)
        if not nnz:
            return empty
        cols = torch.empty(nnz, dtype=torch.int32, device=dev)
        vals = torch.empty(nnz, dtype=torch.float32, device=dev)
        check(lib().mi355_kr_local_qe(*args, cols.data_ptr(), vals.data_ptr(), nnz, stream_ptr(dev)))
    return Csr(offsets, cols, vals)


def _kr_score(query: Csr, gallery: Csr, G: int, shortlist_vals: torch.Tensor, shortlist_idx: torch.Tensor, lam: float) -> torch.Tensor:
    """s* (Q, K) of every shortlist slot (LOCAL row indices; a slot outside the gallery gets -inf)."""
    sv = _f32c(shortlist_vals, "shortlist_vals")
    si = _lists(shortlist_idx, "shortlist_idx")
    if sv.shape != si.shape:
        raise MI355Error(f"shortlist values {tuple(sv.shape)} and indices {tuple(si.shape)} differ")
    Q, K = si.shape
    out = torch.empty((Q, K), dtype=torch.float32, device=si.device)
    if Q:
        if query.offsets.shape != (Q + 1,) or gallery.offsets.shape != (G + 1,):
            raise MI355Error(f"kr_score: offsets of {query.offsets.shape[0] - 1} query and {gallery.offsets.shape[0] - 1} gallery "
                             f"rows for Q={Q}, G={G}")
        with torch.cuda.device(si.device):
            check(lib().mi355_kr_score(query.offsets.data_ptr(), query.cols.data_ptr() or None, query.vals.data_ptr() or None,
                                       query.cols.numel(), Q, gallery.offsets.data_ptr(), gallery.cols.data_ptr() or None,
                                       gallery.vals.data_ptr() or None, gallery.cols.numel(), G, sv.data_ptr(), si.data_ptr(), K,
                                       float(lam), out.data_ptr(), stream_ptr(si.device)))
    return out


def knn_graph(gal: Gallery, k1: int, block: int = 256):
    """(vals (G, k1) fp32, idx (G, k1) int64): the top-k1 OTHER rows of every resident row, ``block`` rows per search."""
    G = gal.rows
    vals = torch.empty((G, k1), dtype=torch.float32, device=gal.device)
    idx = torch.empty((G, k1), dtype=torch.int64, device=gal.device)
    block = max(int(block), 5)                                  # above 4 queries every search takes the tiled kernels
    for q0 in range(0, G, block):
        qn = min(block, G - q0)
        lo = q0 if qn > 4 else max(G - 5, 0)                    # a short last block: the last five rows instead
        hi = q0 + qn
        ex = torch.arange(lo, hi, dtype=torch.int64, device=gal.device)
        v, i = gal.search(gal.data[lo:hi], k1, exclude=ex)
        vals[q0:hi], idx[q0:hi] = v[q0 - lo:], i[q0 - lo:]
    return vals, idx


class RerankIndex:
    """What re-ranking keeps per gallery for one (k1, k2): the kNN graph ``nn`` / ``nv`` (G, k1), ``tau`` (G,) = the k1-th
    neighbour score of each row, and the sparse rows ``V`` (weights over R*(g)) and ``V2`` (their local expansion V'(g))."""

    def __init__(self, gal: Gallery, k1: int, k2: int):
        self.k1, self.k2 = graph_params(gal.rows, k1, k2)
        self.rows = G = gal.rows
        self.nv, self.nn = gal.knn_graph(self.k1)
        self.tau = self.nv[:, self.k1 - 1].contiguous()
        offsets, cols = _kr_sets(self.nn, self.nn)
        self.V = Csr(offsets, cols, _kr_weights(gal._buf, G, gal._buf, G, gal.dim, offsets, cols))
        self.V2 = _kr_local_qe(self.nn, self.k2, self.V, self.V, G)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.nv, self.nn, self.tau)) + self.V.nbytes + self.V2.nbytes


def _shortlist_search(gal: Gallery, q: torch.Tensor, n: int, ex: torch.Tensor | None):
    """``gal.search(q, n, exclude=ex)`` (LOCAL ``ex``) run with more than 4 queries - a smaller batch is padded with copies of
    its last query - so that it takes the same kernels, and gives the same bits, for every batch size.  Returns the (Q, n) values
    and rows of the queries given."""
    Q = q.shape[0]
    qq, exq = q, ex
    if Q < 5:
        qq = torch.cat([q, q[-1:].expand(5 - Q, -1)])
        exq = None if ex is None else torch.cat([ex, ex[-1:].expand(5 - Q)])
    sv, si = gal.search(qq, n, exclude=exq)
    return sv[:Q], si[:Q]


def _rerank_scores(gal: Gallery, q: torch.Tensor, k1: int, k2: int, lam: float, K: int, ex: torch.Tensor | None):
    """The stages of ``rerank`` for checked arguments and LOCAL ``ex``: (s* (Q, K), shortlist values, shortlist rows, nv, nn).
    The search is ``_shortlist_search``: the same bits for every batch size."""
    G, Q = gal.rows, q.shape[0]
    index = gal.rerank_index(k1, k2)
    sv, si = _shortlist_search(gal, q, max(K, k1), ex)
    nv, nn = sv[:Q, :k1].contiguous(), si[:Q, :k1].contiguous()
    sv, si = sv[:Q, :K].contiguous(), si[:Q, :K].contiguous()
    offsets, cols = _kr_sets(nn, index.nn, nv, index.tau)
    vq = Csr(offsets, cols, _kr_weights(l2_normalize_rows(q, gal.eps), Q, gal._buf, G, gal.dim, offsets, cols))
    vq2 = _kr_local_qe(nn, k2, vq, index.V, G)
    return _kr_score(vq2, index.V2, G, sv, si, lam), sv, si, nv, nn


def rerank(gal: Gallery, queries: torch.Tensor, k: int, *, k1: int = 20, k2: int = 6, lam: float = 0.3,
           shortlist: int | None = None, exclude: torch.Tensor | None = None, idx_offset: int = 0):
    """``Gallery.rerank``: round-1 search, the queries' sparse rows against the gallery's ``RerankIndex``, s* on the shortlist,
    then the library's ``topk`` over the shortlist positions and a gather of their rows."""
    q = _f32c(queries, "queries")
    _check_qg(q, gal._resident())
    k, k1, k2, lam, K = rerank_params(gal.rows, k, k1, k2, lam, shortlist)
    ex = None
    if exclude is not None:
        ex = _int64_on(exclude, "exclude", q.shape[0], q.device) - int(idx_offset)   # local rows; another shard's row: none
    if q.shape[0] == 0:
        return (torch.empty((0, k), dtype=torch.float32, device=q.device), torch.empty((0, k), dtype=torch.int64, device=q.device))
    sstar, _, si, _, _ = _rerank_scores(gal, q, k1, k2, lam, K, ex)
    vals, pos = topk(sstar, k)
    idx = torch.gather(si, 1, pos)
    return vals, torch.where(idx >= 0, idx + int(idx_offset), idx)


def k_reciprocal_rerank(queries: torch.Tensor, gallery_rows: torch.Tensor, k: int, *, k1: int = 20, k2: int = 6, lam: float = 0.3,
                        shortlist: int | None = None, exclude: torch.Tensor | None = None, idx_offset: int = 0,
                        eps: float = _EPS):
    """k-reciprocal re-ranking of ``queries`` (Q, D) against a plain (G, D) tensor: ``Gallery(D).add(gallery_rows).rerank(...)``
    (the graph is built for this call; keep a ``Gallery`` to reuse it).  Returns (values (Q, k) fp32, indices (Q, k) int64)
    like ``cosine_topk``: the top-k of the shortlist by descending s*, ties to the earlier shortlist position."""
    q, g = _f32c(queries, "queries"), _f32c(gallery_rows, "gallery")
    _check_qg(q, g)
    rerank_params(g.shape[0], k, k1, k2, lam, shortlist)
    gal = Gallery(g.shape[1], g.device, capacity=g.shape[0], eps=eps).add(g)
    return gal.rerank(q, k, k1=k1, k2=k2, lam=lam, shortlist=shortlist, exclude=exclude, idx_offset=idx_offset)
