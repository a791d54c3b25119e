"""Result diversification (not in the reference, whose ``distinct_class_topn`` needs labels): maximal marginal relevance (Carbonell
and Goldstein, SIGIR 1998) and its hard-threshold cousin, greedy near-duplicate suppression, over a query's shortlist.

Per query: the shortlist search of ``rerank`` (the same helper, hence the same bits at any batch size), the L x L Gram matrix of
the shortlist's gallery rows on the f16 MFMA, then k greedy picks, each the eligible slot of greatest
``lam * rel - (1 - lam) * max similarity to the picks so far`` (csrc/diversify.hip, definitions in include/mi355_retrieval.h).
``dedup=t`` makes a slot ineligible once it is within ``t`` of a pick; ``lam=1`` with ``dedup`` is the label-free form of the
"first n distinct classes" walk, ``lam=1`` without it the plain search order.

* ``_dv_gram`` ...... S (Q, L, L) fp32 of the rows in ``idx``                 (mi355_shortlist_gram)
* ``_dv_select`` .... the picks' cosine scores, rows, MMR values and counts   (mi355_mmr_select)

These staged wrappers take and return device tensors, so a test can feed each step fixed inputs.  Nothing here reads a result
back to the host.  Out of scope: ``ShardedGallery`` (a shortlist spans the shards) and the compressed galleries (their rows are
not fp16 operands)."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import MI355Error, check, lib, stream_ptr
from .rank import _DTYPES, _EPS, Gallery, _check_qg, _f32c, _int64_on, _is_int
from .rerank import MAX_SHORTLIST, _lists, _shortlist_search

GRAM_SCRATCH_BYTES = 256 << 20       # the most the Gram matrices of one block of queries may take


def _lam(lam) -> float:
    try:
        lam = float(lam)
    except (TypeError, ValueError):
        raise MI355Error(f"lam must be a float in [0, 1], got {lam!r}") from None
    if not np.isfinite(lam) or not 0.0 <= lam <= 1.0:
        raise MI355Error(f"lam must be a finite float in [0, 1], got {lam!r}")
    return lam


def _dedup(dedup):
    """None, or the threshold as a float that is finite in fp32 (what the kernel compares with)."""
    if dedup is None:
        return None
    try:
        d = float(dedup)
    except (TypeError, ValueError):
        raise MI355Error(f"dedup must be None or a finite float, got {dedup!r}") from None
    with np.errstate(over="ignore"):
        if isinstance(dedup, bool) or not np.isfinite(d) or not np.isfinite(np.float32(d)):
            raise MI355Error(f"dedup must be None or a finite float, got {dedup!r}")
    return d


def diversify_params(G: int, k, lam=0.7, dedup=None, shortlist=None, block=None):
    """(k, lam, dedup, L, block) checked: k >= 1, lam a finite float in [0, 1], dedup None or a finite float, the shortlist
    k <= L <= min(G, 1024) (default min(G, max(10 k, 100), 1024)), and the number of queries whose Gram matrices are held at a time:
    ``block`` >= 1, by default as many as fit 256 MiB (64 at L = 1024)."""
    lam, dedup = _lam(lam), _dedup(dedup)
    if not _is_int(k) or int(k) < 1:
        raise MI355Error(f"selected index k out of range: k={k!r}, gallery rows={G}")
    k = int(k)
    top = min(G, MAX_SHORTLIST)
    L = min(G, max(10 * k, 100), MAX_SHORTLIST) if shortlist is None else shortlist
    if not _is_int(L) or not k <= int(L) <= top:
        raise MI355Error(f"shortlist must be an integer with k={k} <= shortlist <= min(gallery rows, {MAX_SHORTLIST}) = {top}, "
                         f"got {L!r}")
    L = int(L)
    if block is None:
        block = max(GRAM_SCRATCH_BYTES // (4 * L * L), 1)
    elif not _is_int(block) or int(block) < 1:
        raise MI355Error(f"block must be an integer >= 1, got {block!r}")
    return k, lam, dedup, L, int(block)


def _gallery(gal) -> Gallery:
    if not isinstance(gal, Gallery):
        raise MI355Error(f"diversify reads the fp32 or fp16 rows of a Gallery (prepared or not); a {type(gal).__name__} is not "
                         "supported")
    return gal


def _shortlist_idx(idx: torch.Tensor) -> torch.Tensor:
    idx = _lists(idx, "idx")
    if not 1 <= idx.shape[1] <= MAX_SHORTLIST:
        raise MI355Error(f"shortlist L={idx.shape[1]} outside [1, {MAX_SHORTLIST}]")
    return idx


def _dv_gram(gal: Gallery, idx: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """S (Q, L, L) fp32: the dot products of the gallery rows ``idx`` (Q, L) int64 LOCAL rows names, taken from the fp16 values
    of the resident rows (a prepared gallery: of its fp32 rows); 0 wherever either slot is a pad or outside the gallery."""
    gal = _gallery(gal)
    idx = _shortlist_idx(idx)
    if idx.device != gal.device:
        raise MI355Error(f"idx is on {idx.device} but the gallery lives on {gal.device}")
    if gal.rows < 1:
        raise MI355Error("the gallery holds no rows")
    Q, L = idx.shape
    if out is None:
        out = torch.empty((Q, L, L), dtype=torch.float32, device=idx.device)
    if Q:
        with torch.cuda.device(idx.device):
            check(lib().mi355_shortlist_gram(gal._buf.data_ptr(), _DTYPES[gal.dtype], gal._ld, gal.rows, gal.dim, idx.data_ptr(), Q, L,
                                             out.data_ptr(), stream_ptr(idx.device)))
    return out


def _dv_select(rel: torch.Tensor, idx: torch.Tensor, gram: torch.Tensor, k: int, lam: float = 0.7, dedup=None, idx_offset: int = 0,
               out=None):
    """(cosine scores (Q, k) fp32, rows + idx_offset (Q, k) int64, MMR values (Q, k) fp32, picks (Q,) int32) of the greedy selection
    over ``rel`` / ``idx`` (Q, L), a search's output with LOCAL rows, and ``gram`` (Q, L, L) of ``_dv_gram``."""
    idx = _shortlist_idx(idx)
    rel, gram = _f32c(rel, "rel"), _f32c(gram, "gram")
    Q, L = idx.shape
    if rel.shape != idx.shape or gram.shape != (Q, L, L) or rel.device != idx.device or gram.device != idx.device:
        raise MI355Error(f"rel must be {(Q, L)} and gram {(Q, L, L)} on {idx.device}, got {tuple(rel.shape)} on {rel.device} and "
                         f"{tuple(gram.shape)} on {gram.device}")
    lam, dedup = _lam(lam), _dedup(dedup)
    if not _is_int(k) or not 1 <= int(k) <= L:
        raise MI355Error(f"k must be an integer in [1, shortlist={L}], got {k!r}")
    k, dev = int(k), idx.device
    if out is None:
        out = (torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev),
               torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q,), dtype=torch.int32, device=dev))
    if Q:
        with torch.cuda.device(dev):
            check(lib().mi355_mmr_select(rel.data_ptr(), idx.data_ptr(), gram.data_ptr(), Q, L, k, lam,
                                         float("nan") if dedup is None else dedup, int(idx_offset), out[0].data_ptr(),
                                         out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), stream_ptr(dev)))
    return out


def diversify(gal: Gallery, queries: torch.Tensor, k: int, *, lam: float = 0.7, dedup=None, shortlist: int | None = None,
              exclude: torch.Tensor | None = None, idx_offset: int = 0, stats: bool = False, block: int | None = None):
    """``Gallery.diversify``: the shortlist search, then per block of queries the shortlist Gram matrices and the greedy
    selection.  A query's result does not depend on the batch or on the blocking."""
    gal = _gallery(gal)
    q = _f32c(queries, "queries")
    _check_qg(q, gal._resident())
    k, lam, dedup, L, block = diversify_params(gal.rows, k, lam, dedup, shortlist, block)
    ex = None
    if exclude is not None:
        ex = _int64_on(exclude, "exclude", q.shape[0], q.device) - int(idx_offset)   # local rows; another shard's row: none
    Q, dev = q.shape[0], q.device
    out = (torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int64, device=dev),
           torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q,), dtype=torch.int32, device=dev))
    if Q:
        sv, si = _shortlist_search(gal, q, L, ex)
        sv, si = sv.contiguous(), si.contiguous()
        scratch = torch.empty((min(block, Q), L, L), dtype=torch.float32, device=dev)
        for q0 in range(0, Q, block):
            q1 = min(q0 + block, Q)
            gram = _dv_gram(gal, si[q0:q1], scratch[: q1 - q0])
            _dv_select(sv[q0:q1], si[q0:q1], gram, k, lam, dedup, idx_offset, tuple(t[q0:q1] for t in out))
    return out if stats else out[:2]


def mmr_rerank(queries: torch.Tensor, gallery_rows: torch.Tensor, k: int, *, lam: float = 0.7, dedup=None,
               shortlist: int | None = None, exclude: torch.Tensor | None = None, idx_offset: int = 0, stats: bool = False,
               block: int | None = None, eps: float = _EPS):
    """MMR diversification of ``queries`` (Q, D) against a plain (G, D) tensor: ``Gallery(D).add(gallery_rows).diversify(...)``.
    Returns (cosine scores (Q, k) fp32, indices (Q, k) int64) in pick order; the scores are not monotone."""
    q, g = _f32c(queries, "queries"), _f32c(gallery_rows, "gallery")
    _check_qg(q, g)
    diversify_params(g.shape[0], k, lam, dedup, shortlist, block)
    gal = Gallery(g.shape[1], g.device, capacity=g.shape[0], eps=eps).add(g)
    return gal.diversify(q, k, lam=lam, dedup=dedup, shortlist=shortlist, exclude=exclude, idx_offset=idx_offset, stats=stats,
                         block=block)
