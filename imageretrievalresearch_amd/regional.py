"""Regional MaxSim re-ranking (not in the reference): an image is kept as its R regional vectors - what ``aggregate(fm, "rmac" |
"regions", return_regions=True)`` returns - and a query image is scored against a candidate by matching every query region to its
best region of the candidate and averaging the maxima (Razavian et al. 2016; Tolias et al., ICLR 2016, section 5; the "late
interaction" of ColBERT).  A global descriptor sums the regions, so an object that fills one of R regions of a cluttered image
carries 1 / R of it; the regional score finds the object's region.  It is run as a re-ranker over the shortlist of a global
search, where ``Gallery.rerank`` and ``Gallery.diffuse`` stand.

``RegionGallery`` stores ``fp16(l2_normalize_rows(v))`` per region in the fp16 ``Gallery`` row layout; queries are rounded the
same way, so both sides of every product are fp16 values and every product is exact in fp32.  For one (query, row) pair

    s[i][j] = sum_d float(qh[i][d]) * float(gh[j][d])    (fp32)
    m[i] = max_j s[i][j],  a[i] = the lowest j that attains it
    score = sum_i w[i] * m[i]                            (fp32, ascending i)

on ``v_mfma_f32_16x16x32_f16`` (csrc/regional.hip; definitions in include/mi355_retrieval.h).  The bits of a pair depend on the
query's codes, its weights and the row alone.  Nothing here reads a result back to the host.  Out of scope: ``ShardedGallery``,
int8 / fp4 region codes, a symmetric (two-way) score."""
from __future__ import annotations

import torch

from . import rank as _rank
from ._lib import MI355Error, check, lib, require_cuda, stream_ptr
from .rerank import MAX_SHORTLIST, _shortlist_search

MAX_REGIONS = 64     # MI355_REGION_MAX_REGIONS
MAX_DIM = 65536
MAX_LIST = MAX_SHORTLIST
LDS_BYTES = 64 * 1024
_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def lds_bytes(Rq: int, dim: int) -> int:
    """The LDS one workgroup keeps a query's codes in at (Rq, dim) (``mi355_region_scores_lds_bytes``: the sizer the entry itself
    checks with); 0 for a shape outside the limits."""
    return int(lib().mi355_region_scores_lds_bytes(int(Rq), int(dim)))


def rerank_params(rows: int, k, shortlist=None):
    """(k, L) checked against a gallery of ``rows`` rows: k >= 1 and the shortlist k <= L <= min(rows, 1024) (default
    min(rows, max(k, 100)))."""
    if not _rank._is_int(k) or int(k) < 1:
        raise MI355Error(f"selected index k out of range: k={k!r}, gallery rows={rows}")
    k = int(k)
    top = min(rows, MAX_LIST)
    L = min(rows, max(k, 100)) if shortlist is None else shortlist
    if not _rank._is_int(L) or not k <= int(L) <= top:
        raise MI355Error(f"shortlist must be an integer with k={k} <= shortlist <= min(gallery rows, {MAX_LIST}) = {top}, "
                         f"got {L!r}")
    return k, int(L)


def _regions_shape(t, name: str, dim: int, count: int | None = None) -> None:
    """``t`` checked as (n, regions, dim) floating-point vectors, wherever they live."""
    if not torch.is_tensor(t):
        raise MI355Error(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype not in _FLOATS:
        raise MI355Error(f"{name} must be float32, float16 or bfloat16, got {t.dtype}")
    if t.dim() != 3 or t.shape[2] != dim:
        raise MI355Error(f"{name} must be (n, regions, {dim}), got {tuple(t.shape)}")
    if count is not None and t.shape[1] != count:
        raise MI355Error(f"{name} must hold {count} regions per row, got {tuple(t.shape)}")
    if not 1 <= t.shape[1] <= MAX_REGIONS:
        raise MI355Error(f"{name}: {t.shape[1]} regions outside [1, {MAX_REGIONS}]")


def _regions(t, name: str, dim: int, count: int | None = None) -> torch.Tensor:
    """``t`` checked as (n, regions, dim) floating-point vectors on the GPU; returns them as contiguous fp32."""
    _regions_shape(t, name, dim, count)
    require_cuda(t, name)
    return t.float().contiguous()


class RegionGallery(_rank._RowStore):
    """Resident regional gallery: ``regions`` vectors of ``dim`` columns per row, each stored as ``fp16(l2_normalize_rows(v))`` in a
    (capacity, regions, ld) buffer, ``ld`` = ``dim`` rounded up to a multiple of 64 with zeros behind ``dim`` - the bits an fp16
    ``Gallery`` stores for the same (n * regions, dim) vectors.  ``scores`` is the regional MaxSim of the module docstring over a
    list of rows per query, ``rerank`` runs it over the shortlist of a global ``Gallery`` of the same rows, ``search`` over every
    row (small galleries), ``pooled`` makes that global gallery from the regions themselves."""

    _NOUN = "RegionGallery"
    _BUFFERS = ("_buf",)

    def __init__(self, dim: int, regions: int, device, capacity: int = 0, eps: float = _rank._EPS):
        super().__init__(dim, device, eps)
        if not _rank._is_int(regions) or not 1 <= int(regions) <= MAX_REGIONS:
            raise MI355Error(f"a RegionGallery needs regions an integer in [1, {MAX_REGIONS}], got {regions!r}")
        if not 1 <= self.dim <= MAX_DIM:
            raise MI355Error(f"a RegionGallery needs 1 <= dim <= {MAX_DIM}, got {dim}")
        self.regions = int(regions)
        self._ld = _rank._f16_stride(self.dim)
        self._buf = torch.empty((max(int(capacity), 0), self.regions, self._ld), dtype=torch.float16, device=self.device)

    def _codes(self, e: torch.Tensor, out: torch.Tensor) -> None:
        """fp16(l2_normalize_rows(e)) of the (n, r, dim) fp32 vectors ``e`` into the (n, r, ld) rows ``out``."""
        n = e.shape[0] * e.shape[1]
        with torch.cuda.device(e.device):
            check(lib().mi355_gallery_to_f16(e.data_ptr(), n, self.dim, 0, self.eps, out.data_ptr(),
                                             _rank._gallery_f16_bytes(n, self.dim), stream_ptr(e.device)))

    def _write(self, e: torch.Tensor, r0: int) -> None:
        self._codes(e, self._buf[r0: r0 + e.shape[0]])

    def add(self, regions: torch.Tensor, labels: torch.Tensor | None = None):
        """``regions`` (n, R, dim) floating-point vectors behind the resident rows, ``labels`` (n,) with them."""
        e = _regions(regions, "regions", self.dim, self.regions)
        if e.device != self.device:
            raise MI355Error(f"regions are on {e.device} but the RegionGallery lives on {self.device}")
        if labels is not None and (not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != e.shape[0]):
            raise MI355Error(f"labels must be a ({e.shape[0]},) tensor")
        return self._append(e, labels)

    @property
    def data(self) -> torch.Tensor:
        """The (rows, R, dim) fp16 unit vectors (a view, without the row padding)."""
        return self._buf[: self.rows, :, : self.dim]

    @property
    def nbytes(self) -> int:
        """Resident footprint in bytes: the buffer at its current capacity, ``capacity * R * ld * 2``."""
        return self._buf.numel() * self._buf.element_size()

    def query_codes(self, query_regions: torch.Tensor) -> torch.Tensor:
        """(Q, Rq, ld) fp16 codes of ``query_regions`` (Q, Rq, dim) fp32 / fp16 / bf16, 1 <= Rq <= 64 whatever R is: normalised and
        rounded as ``add`` does.  The rounding is deliberate: both sides of a product are then fp16 values."""
        return self._query_codes(self._query(query_regions))

    def _query(self, query_regions) -> torch.Tensor:
        e = _regions(query_regions, "query_regions", self.dim)
        if e.device != self.device:
            raise MI355Error(f"query_regions are on {e.device} but the RegionGallery lives on {self.device}")
        return e

    def _query_codes(self, e: torch.Tensor) -> torch.Tensor:
        out = torch.empty((e.shape[0], e.shape[1], self._ld), dtype=torch.float16, device=self.device)
        if e.shape[0]:
            self._codes(e, out)
        return out

    def _weights(self, weights, Q: int, Rq: int, placed: bool = True):
        if weights is None:
            return None
        if not torch.is_tensor(weights):
            raise MI355Error(f"weights must be a tensor, got {type(weights).__name__}")
        if weights.dtype != torch.float32 or tuple(weights.shape) != (Q, Rq):
            raise MI355Error(f"weights must be ({Q}, {Rq}) float32, got {weights.dtype} {tuple(weights.shape)}")
        if not placed:
            return None
        require_cuda(weights, "weights")
        if weights.device != self.device:
            raise MI355Error(f"weights are on {weights.device} but the RegionGallery lives on {self.device}")
        return weights.contiguous()

    def _list(self, idx, Q: int, placed: bool = True):
        if idx is None:
            return None, self.rows
        if not torch.is_tensor(idx):
            raise MI355Error(f"idx must be a tensor, got {type(idx).__name__}")
        if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != Q:
            raise MI355Error(f"idx must be ({Q}, L) int64, got {idx.dtype} {tuple(idx.shape)}")
        if not 1 <= idx.shape[1] <= MAX_LIST:
            raise MI355Error(f"list length L={idx.shape[1]} outside [1, {MAX_LIST}]")
        if not placed:
            return None, idx.shape[1]
        require_cuda(idx, "idx")
        if idx.device != self.device:
            raise MI355Error(f"idx is on {idx.device} but the RegionGallery lives on {self.device}")
        return idx.contiguous(), idx.shape[1]

    def scores(self, query_regions: torch.Tensor, idx: torch.Tensor | None = None, *, weights: torch.Tensor | None = None,
               matches: bool = False):
        """(Q, L) fp32 regional scores of ``query_regions`` (Q, Rq, dim) against the rows ``idx`` (Q, L) int64 names - LOCAL rows,
        1 <= L <= 1024, a row may occur twice, a slot of -1 is a pad and scores -inf (so does any slot outside [0, rows): the
        kernel treats it as a pad and reads nothing) - or against every row (``idx=None``: L = rows, no limit).  ``weights``
        (Q, Rq) fp32, default ``fp32(1) / fp32(Rq)`` each; a zero weight drops a region (ragged queries).  ``matches=True``: also
        (Q, L, Rq) int32, the gallery region that attains each maximum, ties to the lower region, -1 in pad slots."""
        _regions_shape(query_regions, "query_regions", self.dim)
        Q, Rq = query_regions.shape[0], query_regions.shape[1]
        self._weights(weights, Q, Rq, False)                     # every shape and dtype before any device
        self._list(idx, Q, False)
        e = self._query(query_regions)
        w = self._weights(weights, Q, Rq)
        ix, L = self._list(idx, Q)
        if self.rows == 0:
            raise MI355Error("the RegionGallery is empty: add regions first")
        need = lds_bytes(Rq, self.dim)
        if not 0 < need <= LDS_BYTES:
            raise MI355Error(f"Rq={Rq}, dim={self.dim} needs {need} bytes of LDS, outside (0, {LDS_BYTES}]")
        qc = self._query_codes(e)
        out = torch.empty((Q, L), dtype=torch.float32, device=self.device)
        mt = torch.empty((Q, L, Rq), dtype=torch.int32, device=self.device) if matches else None
        if Q:
            with torch.cuda.device(self.device):
                check(lib().mi355_region_scores(qc.data_ptr(), Q, Rq, self._buf.data_ptr(), self.rows, self.regions, self.dim,
                                                self._ld, None if ix is None else ix.data_ptr(), L,
                                                None if w is None else w.data_ptr(), out.data_ptr(),
                                                None if mt is None else mt.data_ptr(), stream_ptr(self.device)))
        return (out, mt) if matches else out

    def _k(self, k, top: int, what: str) -> int:
        if not _rank._is_int(k) or not 1 <= int(k) <= top:
            raise MI355Error(f"selected index k out of range: k={k!r} outside [1, {top}] ({what})")
        return int(k)

    def _exclude(self, exclude, Q: int, idx_offset: int):
        if exclude is None:
            return None
        return _rank._int64_on(exclude, "exclude", Q, self.device) - int(idx_offset)     # local rows; another shard's row: none

    def search(self, query_regions: torch.Tensor, k: int, *, weights: torch.Tensor | None = None,
               exclude: torch.Tensor | None = None, idx_offset: int = 0):
        """Top-k of ``scores(query_regions)`` over every row: (values (Q, k) fp32, indices (Q, k) int64) by the library's ``topk``
        (descending, ties to the lower row), ``exclude`` (Q,) one row per query left out, ``idx_offset`` added to the rows; pads
        are (-inf, -1).  It keeps a Q x rows slab of scores and reads every row's regions: meant for galleries of up to tens of
        thousands of rows - over a large one, ``rerank`` a shortlist."""
        k = self._k(k, min(_rank._MAX_K, self.rows), f"min({_rank._MAX_K}, rows)")
        _regions_shape(query_regions, "query_regions", self.dim)
        Q = query_regions.shape[0]
        ex = self._exclude(exclude, Q, idx_offset)
        s = self.scores(query_regions, weights=weights)
        if ex is not None and Q:
            inside = (ex >= 0) & (ex < self.rows)
            col = ex.clamp(0, self.rows - 1)[:, None]
            s.scatter_(1, col, torch.where(inside[:, None], torch.full_like(s[:, :1], float("-inf")), s.gather(1, col)))
        vals, idx = _rank.topk(s, k)
        return vals, torch.where(vals == float("-inf"), torch.full_like(idx, -1), idx + int(idx_offset))

    def rerank(self, gallery, queries: torch.Tensor, query_regions: torch.Tensor, k: int, *, shortlist: int | None = None,
               weights: torch.Tensor | None = None, exclude: torch.Tensor | None = None, idx_offset: int = 0, matches: bool = False):
        """``gallery.search(queries, shortlist)`` re-scored by ``scores``: the top-k of the shortlist by descending regional score as
        (values (Q, k) fp32, indices (Q, k) int64 [, matches (Q, k, Rq) int32]), ties to the earlier shortlist position, pads
        (-inf, -1) last.  ``gallery``: a ``Gallery`` of the same number of rows on the same device, row r the global descriptor of
        the image whose regions are row r here (its ``dim`` is free; ``pooled()`` makes one); ``queries`` (Q, gallery.dim) the
        global descriptors of the query images.  ``shortlist``: k <= shortlist <= min(rows, 1024), default min(rows, max(k, 100));
        ``exclude`` / ``idx_offset`` as in ``Gallery.search``."""
        if not isinstance(gallery, _rank.Gallery):
            raise MI355Error(f"gallery must be a Gallery of the same rows, got {type(gallery).__name__}")
        if gallery.device != self.device:
            raise MI355Error(f"gallery is on {gallery.device} but the RegionGallery lives on {self.device}")
        if len(gallery) != self.rows:
            raise MI355Error(f"gallery holds {len(gallery)} rows, the RegionGallery {self.rows}")
        k, L = rerank_params(self.rows, k, shortlist)
        if not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != gallery.dim:
            raise MI355Error(f"queries must be (Q, {gallery.dim}), the global descriptors of the query images")
        if not torch.is_tensor(query_regions) or query_regions.dim() != 3 or query_regions.shape[0] != queries.shape[0]:
            raise MI355Error(f"query_regions must be ({queries.shape[0]}, Rq, {self.dim}), one set of regions per query")
        Q, Rq = query_regions.shape[0], query_regions.shape[1]
        _regions_shape(query_regions, "query_regions", self.dim)
        self._weights(weights, Q, Rq, False)
        e = self._query(query_regions)
        self._weights(weights, Q, Rq)
        q = _rank._f32c(queries, "queries")
        _rank._check_qg(q, gallery._resident())
        ex = self._exclude(exclude, Q, idx_offset)
        if Q == 0:
            out = (torch.empty((0, k), dtype=torch.float32, device=self.device), torch.empty((0, k), dtype=torch.int64, device=self.device))
            return out + (torch.empty((0, k, Rq), dtype=torch.int32, device=self.device),) if matches else out
        _, si = _shortlist_search(gallery, q, L, ex)
        si = si.contiguous()
        got = self.scores(e, si, weights=weights, matches=matches)
        s, mt = got if matches else (got, None)
        vals, pos = _rank.topk(s, k)
        idx = torch.gather(si, 1, pos)
        idx = torch.where(idx >= 0, idx + int(idx_offset), idx)
        if not matches:
            return vals, idx
        return vals, idx, torch.gather(mt, 1, pos[:, :, None].expand(-1, -1, Rq))

    def pooled(self, dtype: torch.dtype = torch.float32) -> "_rank.Gallery":
        """A ``Gallery`` (``dtype`` fp32 or fp16, same eps, labels copied) whose row r is the sum of row r's stored regions in region
        order, normalised - ``aggregate._sum_regions(self.data.float(), True, eps)``, the R-MAC descriptor of the stored regions:
        who keeps only regions builds the shortlist gallery of ``rerank`` from it."""
        from .aggregate import _sum_regions
        out = _rank.Gallery(self.dim, self.device, capacity=self.rows, eps=self.eps, dtype=dtype)
        out.labels = None if self.labels is None else self.labels.clone()
        if self.rows:
            rows = _sum_regions(self.data.float().contiguous(), True, self.eps)
            if dtype == torch.float32:
                out._buf[: self.rows].copy_(rows)
            else:                                                    # the rows are normalised: rounded as add would round them
                with torch.cuda.device(self.device):
                    check(lib().mi355_gallery_to_f16(rows.data_ptr(), self.rows, self.dim, 1, self.eps, out._buf.data_ptr(),
                                                     _rank._gallery_f16_bytes(self.rows, self.dim), stream_ptr(self.device)))
        out.rows = self.rows
        return out


def maxsim(query_regions: torch.Tensor, gallery_regions: torch.Tensor, weights: torch.Tensor | None = None, eps: float = _rank._EPS):
    """(Q, G) fp32 regional scores of ``query_regions`` (Q, Rq, dim) against ``gallery_regions`` (G, R, dim): ``RegionGallery(dim,
    R).add(gallery_regions).scores(query_regions, weights=weights)`` (the codes are made for this call; keep a ``RegionGallery`` to
    reuse them)."""
    if not torch.is_tensor(gallery_regions) or gallery_regions.dim() != 3:
        raise MI355Error("gallery_regions must be a (G, R, dim) tensor")
    require_cuda(gallery_regions, "gallery_regions")
    G, R, dim = gallery_regions.shape
    rg = RegionGallery(dim, R, gallery_regions.device, capacity=G, eps=eps).add(gallery_regions)
    return rg.scores(query_regions, weights=weights)
