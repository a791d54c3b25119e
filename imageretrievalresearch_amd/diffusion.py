"""Diffusion re-ranking of search results (Iscen, Tolias, Avrithis, Furon and Chum, CVPR 2017; not in the reference), truncated
to a query's shortlist as in Yang, Hinami, Matsui, Ly and Satoh, AAAI 2019.

Offline, once per gallery and (kd, gamma), a ``DiffusionIndex``: the mutual edges of ``Gallery.knn_graph(kd)`` with the affinity
``min(a(i -> j), a(j -> i))``, ``a = max(score, 0)^gamma``, normalised symmetrically to ``S = D^-1/2 W D^-1/2`` and kept as
fixed-width rows.  Online, per query: the shortlist search of ``rerank`` (the same helper), a source vector ``y`` on the first
``kq`` shortlist slots, and ``(I - alpha S_L) f = y`` solved by conjugate gradients on the sub-graph ``S_L`` that the shortlist
induces - one workgroup per query, the graph's local positions and the search direction in LDS (csrc/diffusion.hip, definitions
in include/mi355_retrieval.h).  A row that is far from the query by cosine but joined to it by a chain of near neighbours inside
the shortlist moves to the front.  No (Q + G)^2 or G x G object exists at any point.

* ``_df_graph`` ..... (cols, vals, deg) of a kNN graph              (mi355_diffusion_graph, two launches)
* ``_df_source`` .... y = max(score, 0)^gamma on the first kq slots (mi355_diffusion_source)
* ``_df_solve`` ..... f (and the iterations done) of every query    (mi355_diffusion_solve), then the library's ``topk``

These staged wrappers take and return device tensors, so a test can feed each step fixed inputs.  Nothing here reads a result
back to the host.  Out of scope: ``ShardedGallery`` (the graph spans the shards)."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import MI355Error, check, lib, require_cuda, stream_ptr
from .rank import _EPS, Gallery, _check_qg, _f32c, _int64_on, _is_int, topk
from .rerank import MAX_SHORTLIST, _int_in, _lists, _shortlist_search, graph_params

MAX_KD = 32          # MI355_DIFFUSION_MAX_KD
MAX_GAMMA, MAX_ITERS = 8, 64
LDS_BYTES = 160 * 1024


def _alpha(alpha) -> float:
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise MI355Error(f"alpha must be a float in (0, 1), got {alpha!r}") from None
    # the kernel takes alpha as fp32: what rounds to 0 or 1 there is outside the open interval too
    if not np.isfinite(alpha) or not 0.0 < float(np.float32(alpha)) < 1.0:
        raise MI355Error(f"alpha must be a finite float in (0, 1), got {alpha!r}")
    return alpha


def index_params(G: int, kd=20, gamma=3):
    """(kd, gamma) checked against a gallery of G rows: ``graph_params`` (1 <= kd <= 32, kd < G) and gamma an integer in [1, 8]."""
    kd, _ = graph_params(G, kd)
    return kd, _int_in("gamma", gamma, 1, MAX_GAMMA)


def diffusion_params(G: int, k, kd=20, kq=10, alpha=0.99, gamma=3, iters=20, shortlist=None):
    """(k, kd, kq, alpha, gamma, iters, L) checked: ``index_params``, alpha a finite float in (0, 1), iters in [1, 64], k >= 1, the
    shortlist k <= L <= min(G, 1024) (default min(G, max(k, 200))) and 1 <= kq <= L."""
    kd, gamma = index_params(G, kd, gamma)
    alpha = _alpha(alpha)
    iters = _int_in("iters", iters, 1, MAX_ITERS)
    if not _is_int(k) or int(k) < 1:
        raise MI355Error(f"selected index k out of range: k={k!r}, gallery rows={G}")
    k = int(k)
    top = min(G, MAX_SHORTLIST)
    L = min(G, max(k, 200)) if shortlist is None else shortlist
    if not _is_int(L) or not k <= int(L) <= top:
        raise MI355Error(f"shortlist must be an integer with k={k} <= shortlist <= min(gallery rows, {MAX_SHORTLIST}) = {top}, "
                         f"got {L!r}")
    L = int(L)
    if not _is_int(kq) or not 1 <= int(kq) <= L:
        raise MI355Error(f"kq must be an integer in [1, shortlist={L}], got {kq!r}")
    return k, kd, int(kq), alpha, gamma, iters, L


def lds_bytes(L: int, kd: int) -> int:
    """The LDS one query's workgroup takes at (L, kd) (``mi355_diffusion_lds_bytes``: the sizer the entry itself checks with)."""
    return int(lib().mi355_diffusion_lds_bytes(int(L), int(kd)))


def _df_graph(nn: torch.Tensor, nv: torch.Tensor, gamma: int = 3):
    """(cols (G, kd) int32, vals (G, kd) fp32, deg (G,) fp32) of the kNN graph ``nn`` (G, kd) int64 / ``nv`` (G, kd) fp32."""
    nn = _lists(nn, "nn")
    nv = _f32c(nv, "nv")
    G, kd = nn.shape
    if nv.shape != nn.shape or nv.device != nn.device:
        raise MI355Error(f"nv must be {tuple(nn.shape)} on {nn.device}, got {tuple(nv.shape)} on {nv.device}")
    kd, gamma = index_params(G, kd, gamma)
    dev = nn.device
    cols = torch.empty((G, kd), dtype=torch.int32, device=dev)
    vals = torch.empty((G, kd), dtype=torch.float32, device=dev)
    deg = torch.empty((G,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().mi355_diffusion_graph(nn.data_ptr(), nv.data_ptr(), G, kd, gamma, cols.data_ptr(), vals.data_ptr(),
                                          deg.data_ptr(), stream_ptr(dev)))
    return cols, vals, deg


def _shortlist_pair(shortlist_idx: torch.Tensor, other: torch.Tensor, name: str):
    si = _lists(shortlist_idx, "shortlist_idx")
    other = _f32c(other, name)
    if other.shape != si.shape or other.device != si.device:
        raise MI355Error(f"{name} must be {tuple(si.shape)} on {si.device}, got {tuple(other.shape)} on {other.device}")
    if not 1 <= si.shape[1] <= MAX_SHORTLIST:
        raise MI355Error(f"shortlist L={si.shape[1]} outside [1, {MAX_SHORTLIST}]")
    return si, other


def _df_source(shortlist_vals: torch.Tensor, shortlist_idx: torch.Tensor, kq: int, gamma: int = 3) -> torch.Tensor:
    """y (Q, L) fp32: ``max(shortlist_vals, 0)^gamma`` on the first ``kq`` slots that hold a row, 0 elsewhere."""
    si, sv = _shortlist_pair(shortlist_idx, shortlist_vals, "shortlist_vals")
    Q, L = si.shape
    kq, gamma = _int_in("kq", kq, 1, L), _int_in("gamma", gamma, 1, MAX_GAMMA)
    y = torch.empty((Q, L), dtype=torch.float32, device=si.device)
    if Q:
        with torch.cuda.device(si.device):
            check(lib().mi355_diffusion_source(sv.data_ptr(), si.data_ptr(), Q, L, kq, gamma, y.data_ptr(), stream_ptr(si.device)))
    return y


def _df_solve(cols: torch.Tensor, vals: torch.Tensor, shortlist_idx: torch.Tensor, y: torch.Tensor, alpha: float = 0.99,
              iters: int = 20):
    """(f (Q, L) fp32, iterations (Q,) int32): ``(I - alpha S_L) f = y`` of every query by at most ``iters`` CG iterations on
    the index rows ``cols`` / ``vals`` (G, kd) restricted to ``shortlist_idx`` (Q, L) int64 LOCAL rows; a pad slot gets -inf."""
    for t, name in ((cols, "cols"), (vals, "vals")):
        require_cuda(t, name)
    if cols.dim() != 2 or cols.dtype != torch.int32 or vals.dtype != torch.float32 or vals.shape != cols.shape \
            or vals.device != cols.device:
        raise MI355Error(f"cols must be (G, kd) int32 and vals (G, kd) fp32 on one device, got {cols.dtype} {tuple(cols.shape)} / "
                         f"{vals.dtype} {tuple(vals.shape)}")
    cols, vals = cols.contiguous(), vals.contiguous()
    G, kd = cols.shape
    si, y = _shortlist_pair(shortlist_idx, y, "y")
    if si.device != cols.device:
        raise MI355Error(f"shortlist_idx is on {si.device} but the index on {cols.device}")
    Q, L = si.shape
    if G < 1 or not 1 <= kd <= MAX_KD:
        raise MI355Error(f"the index rows must be (G >= 1, kd in [1, {MAX_KD}]), got {tuple(cols.shape)}")
    alpha, iters = _alpha(alpha), _int_in("iters", iters, 1, MAX_ITERS)
    need = lds_bytes(L, kd)
    if not 0 < need <= LDS_BYTES:
        raise MI355Error(f"L={L}, kd={kd} needs {need} bytes of LDS, outside (0, {LDS_BYTES}]")
    f = torch.empty((Q, L), dtype=torch.float32, device=si.device)
    its = torch.empty((Q,), dtype=torch.int32, device=si.device)
    if Q:
        with torch.cuda.device(si.device):
            check(lib().mi355_diffusion_solve(cols.data_ptr(), vals.data_ptr(), G, kd, si.data_ptr(), y.data_ptr(), Q, L, alpha, iters,
                                              f.data_ptr(), its.data_ptr(), stream_ptr(si.device)))
    return f, its


class DiffusionIndex:
    """What diffusion keeps per gallery for one (kd, gamma): the kNN graph ``nn`` / ``nv`` (G, kd) and the normalised affinity
    rows ``cols`` (G, kd) int32 (-1: no mutual edge), ``vals`` (G, kd) fp32 and ``deg`` (G,) fp32."""

    def __init__(self, gal: Gallery, kd: int = 20, gamma: int = 3):
        self.kd, self.gamma = index_params(gal.rows, kd, gamma)
        self.rows = gal.rows
        self.nv, self.nn = gal.knn_graph(self.kd)
        self.cols, self.vals, self.deg = _df_graph(self.nn, self.nv, self.gamma)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.nv, self.nn, self.cols, self.vals, self.deg))


def _diffusion_scores(gal: Gallery, q: torch.Tensor, kd: int, kq: int, alpha: float, gamma: int, iters: int, L: int,
                      ex: torch.Tensor | None):
    """The stages of ``diffuse`` for checked arguments and LOCAL ``ex``: (f (Q, L), iterations (Q,), shortlist values, rows)."""
    index = gal.diffusion_index(kd, gamma)
    sv, si = _shortlist_search(gal, q, L, ex)
    sv, si = sv.contiguous(), si.contiguous()
    f, its = _df_solve(index.cols, index.vals, si, _df_source(sv, si, kq, gamma), alpha, iters)
    return f, its, sv, si


def diffuse(gal: Gallery, queries: torch.Tensor, k: int, *, kd: int = 20, kq: int = 10, alpha: float = 0.99, gamma: int = 3,
            iters: int = 20, shortlist: int | None = None, exclude: torch.Tensor | None = None, idx_offset: int = 0,
            stats: bool = False):
    """``Gallery.diffuse``: the shortlist search, the source vector, the CG solve on the gallery's ``DiffusionIndex``, then the
    library's ``topk`` over the shortlist positions and a gather of their rows."""
    q = _f32c(queries, "queries")
    _check_qg(q, gal._resident())
    k, kd, kq, alpha, gamma, iters, L = diffusion_params(gal.rows, k, kd, kq, alpha, gamma, iters, shortlist)
    ex = None
    if exclude is not None:
        ex = _int64_on(exclude, "exclude", q.shape[0], q.device) - int(idx_offset)   # local rows; another shard's row: none
    if q.shape[0] == 0:
        out = (torch.empty((0, k), dtype=torch.float32, device=q.device), torch.empty((0, k), dtype=torch.int64, device=q.device))
        return out + (torch.empty((0,), dtype=torch.int32, device=q.device),) if stats else out
    f, its, _, si = _diffusion_scores(gal, q, kd, kq, alpha, gamma, iters, L, ex)
    vals, pos = topk(f, k)
    idx = torch.gather(si, 1, pos)
    idx = torch.where(idx >= 0, idx + int(idx_offset), idx)
    return (vals, idx, its) if stats else (vals, idx)


def diffusion_rerank(queries: torch.Tensor, gallery_rows: torch.Tensor, k: int, *, kd: int = 20, kq: int = 10, alpha: float = 0.99,
                     gamma: int = 3, iters: int = 20, shortlist: int | None = None, exclude: torch.Tensor | None = None,
                     idx_offset: int = 0, stats: bool = False, eps: float = _EPS):
    """Diffusion re-ranking of ``queries`` (Q, D) against a plain (G, D) tensor: ``Gallery(D).add(gallery_rows).diffuse(...)`` (the
    index is built for this call; keep a ``Gallery`` to reuse it).  Returns (values (Q, k) fp32, indices (Q, k) int64) like
    ``cosine_topk``: the top-k of the shortlist by descending f, ties to the earlier shortlist position."""
    q, g = _f32c(queries, "queries"), _f32c(gallery_rows, "gallery")
    _check_qg(q, g)
    diffusion_params(g.shape[0], k, kd, kq, alpha, gamma, iters, shortlist)
    gal = Gallery(g.shape[1], g.device, capacity=g.shape[0], eps=eps).add(g)
    return gal.diffuse(q, k, kd=kd, kq=kq, alpha=alpha, gamma=gamma, iters=iters, shortlist=shortlist, exclude=exclude,
                       idx_offset=idx_offset, stats=stats)
