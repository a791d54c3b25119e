"""Row-sharded gallery across the GPUs of one node.

One process per GPU (``torch.distributed``; backend "nccl" is RCCL on ROCm, xGMI underneath).
The reference has no multi-GPU inference path (inference/inference.py:271 is single-device); this is
the one place the hot path has a real exchange step:

  1. every rank embeds its own images -> its gallery shard is *born* local, rows
     ``[offset[r], offset[r+1])`` of the global gallery; no collective during embedding
  2. queries are replicated with one all-gather of (Q_local, D) fp32 (1.5 MB at Q=256)
  3. each rank runs cosine + top-k over its shard (k <= 8: selected inside the GEMM epilogue, no score slab)
     -> (Q, k) {f32 score, i32 LOCAL index}
  4. ONE all-gather of the packed candidates (Q*k*8 bytes per rank: KBs, so latency- not link-bound; RCCL picks
     a direct one-hop exchange at this size, a ring would be 7 serial xGMI hops for nothing)
  5. every rank adds the shard offsets (a device tensor, no host sync) and merges world*k candidates per query
     (both inside ``mi355_merge_packed_topk``) with the same ordering rule (higher score, then LOWER global index) -> identical to the single-GPU result,
     bit for bit.

world_size == 1 never touches torch.distributed.

Each rank holds ONE ``self.shard``.  Under the default backend (``_HipOps``) it is the ``rank._Rows`` that ``_HipOps.shard``
builds once: the normalised rows as fp32 or fp16, with the bf16 planes when ``prepared=True``; ``rank``'s one function per
operation picks the kernel from it.  ``self.local`` is its (rows, dim) view, ``self.labels`` the shard's labels (owned here,
handed to each operation).  The backend interface is ``normalize``, ``local_topk(queries, shard, k, idx_offset, **filter)``,
``pack``, ``merge_packed``, ``clear_pads``, ``roc_hist``, ``roc_finalize``, ``local_range``, ``qe_slab``, ``expand`` and
``moments``; a test may inject a CPU backend that implements the ones it drives.  A backend without ``shard`` keeps what its
``normalize`` returns as the shard, fp32 only.  The filtered search, the range search and the verification ROC share one
query exchange (``_exchange_queries``), the plain and the filtered search one candidate exchange (``_exchange_candidates``).
"""
from __future__ import annotations

import torch

from . import rank as _rank
from ._lib import MI355Error



_SHARD_LABELS = "the shard labels: ShardedGallery(..., labels=)"


class _HipOps:
    """Default compute backend: the HIP library.  ``shard`` builds the resident shard once; every method that takes it in
    the place of the normalised gallery rows also takes a bare normalised fp32 (rows, dim) tensor there.  (Tests inject a
    CPU backend to exercise the collective plumbing under gloo without a GPU; the product path is always this one.)"""

    @staticmethod
    def shard(local_rows, dtype, prepared):
        """The shard as ``rank._Rows``: the normalised rows as fp32 or fp16 (half the bytes, searched with the f16 kernel), and
        with ``prepared`` also the cosine GEMM's bf16 planes (+6 B per element; same results bit for bit)."""
        g = _rank.Gallery(local_rows.shape[1], local_rows.device, capacity=local_rows.shape[0], dtype=dtype).add(local_rows)
        return (g.prepare() if prepared else g)._resident()

    @staticmethod
    def local_topk(queries, shard, k, idx_offset, **filt):
        # filt (filtered searches only): query_labels, gallery_labels, label_filter, exclude
        return _rank._topk(queries, _rank._Rows.of(shard, True), k, idx_offset=idx_offset, **filt)

    @staticmethod
    def roc_hist(queries, query_labels, shard, gallery_labels, exclude, idx_offset, thr):
        """The (2, T + 1) int64 pair histogram of ``queries`` against this shard (rows [idx_offset, ...) of the gallery)."""
        return _rank._roc_hist(queries, query_labels, _rank._Rows.of(shard, True), gallery_labels, exclude, idx_offset, thr)

    @staticmethod
    def local_range(queries, shard, threshold, idx_offset, **filt):
        """``cosine_range`` of ``queries`` against this shard (rows [idx_offset, ...) of the gallery): a ``RangeResult`` with
        GLOBAL indices.  filt: query_labels, gallery_labels, label_filter, exclude."""
        return _rank._range(queries, _rank._Rows.of(shard, True), threshold, idx_offset=idx_offset, **filt)

    @staticmethod
    def roc_finalize(hist, thr):
        return _rank._roc_finalize(hist, thr)

    @staticmethod
    def clear_pads(vals, idx, lo, hi):
        return _rank.clear_pads(vals, idx, lo, hi)

    @staticmethod
    def pack(vals, idx, Q, k, device):
        return _rank.pack_candidates(vals, idx, Q, k, device)

    @staticmethod
    def merge_packed(packed, shard_offsets, k):
        return _rank.merge_packed_topk(packed, shard_offsets, k)

    @staticmethod
    def normalize(rows):
        return _rank.l2_normalize_rows(rows)

    @staticmethod
    def qe_slab(idx, lo, local_rows):
        """(Q, n, D) fp32: row (q, j) = this shard's row idx[q, j] - lo widened exactly to fp32 where the shard owns it, +0.0
        elsewhere (the slab every rank contributes to the exchange of alpha query expansion)."""
        Q, n = idx.shape
        rows = local_rows.shape[0]
        slab = torch.zeros((Q, n, local_rows.shape[1]), dtype=torch.float32, device=idx.device)
        loc = idx - lo
        own = (loc >= 0) & (loc < rows)
        if rows:
            slab[own] = local_rows[loc[own]].float()
        return slab

    @staticmethod
    def moments(shard):
        """(sum (D,), outer (D, D)) float64 device tensors of this shard's normalised rows (mi355_embedding_moments)."""
        from .whitening import embedding_moments
        m = embedding_moments(shard)
        return m.sum, m.outer

    @staticmethod
    def expand(base, slab, vals, idx, alpha, eps):
        """mi355_expand_rows of ``base`` (Q, D) raw queries over the exchanged slab as a (Q * n, D) fp32 gallery."""
        Q, n, D = slab.shape
        return _rank._expand_rows(base.contiguous(), True, slab.view(Q * n, D), torch.float32, Q * n, D, vals, idx, alpha, eps)


class ShardedGallery:
    def __init__(self, local_rows: torch.Tensor, group=None, ops=None, labels: torch.Tensor | None = None,
                 prepared: bool = False, dtype: torch.dtype = torch.float32):
        self.ops = ops or _HipOps
        self.group = group
        dist = torch.distributed
        self.world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        self.rank = dist.get_rank(group) if self.world > 1 else 0
        if local_rows.dim() != 2:
            raise MI355Error(f"local gallery shard must be (rows, dim), got {tuple(local_rows.shape)}")
        self.dim = local_rows.shape[1]
        self.device = local_rows.device
        if dtype not in (torch.float32, torch.float16):
            raise MI355Error(f"ShardedGallery dtype must be torch.float32 or torch.float16, got {dtype}")
        if dtype == torch.float16 and prepared:
            raise MI355Error("prepared=True makes bf16 planes of fp32 rows; it does not combine with dtype=torch.float16")
        rows = local_rows.float().contiguous()
        make = getattr(self.ops, "shard", None)
        if make is not None:
            self.shard = make(rows, dtype, prepared)
            self.local = self.shard.data
        elif dtype != torch.float32:
            raise MI355Error(f"dtype={dtype} needs a backend that builds the shard (ops.shard)")
        else:                                   # an injected backend: its normalised fp32 rows are the shard (no planes)
            self.shard = self.local = self.ops.normalize(rows) if rows.shape[0] else rows
        self.labels = None if labels is None else labels.to(self.device, torch.int64)
        if self.world > 1:
            n = torch.tensor([local_rows.shape[0]], dtype=torch.int64, device=self.device)
            allc = torch.empty(self.world, dtype=torch.int64, device=self.device)
            dist.all_gather_into_tensor(allc, n, group=group)
            counts = allc.cpu().tolist()                     # ONE device->host copy for the whole table
        else:
            counts = [int(local_rows.shape[0])]
        if any(c >= 2 ** 31 - 128 for c in counts):
            raise MI355Error("a gallery shard must have fewer than 2^31 rows (candidates carry int32 local indices)")
        self.counts = counts
        self.offsets = [0]
        for c in counts:
            self.offsets.append(self.offsets[-1] + c)
        self.total_rows = self.offsets[-1]
        self._offsets_dev = torch.tensor(self.offsets[:-1], dtype=torch.int64, device=self.device)

    @property
    def offset(self) -> int:
        return self.offsets[self.rank]

    @property
    def prepared(self):
        """The shard's bf16 planes, or None."""
        return getattr(self.shard, "planes", None)

    def _check_filter(self, label_filter, query_labels):
        if label_filter not in (None, "same", "different"):
            raise MI355Error(f'label_filter must be None, "same" or "different", got {label_filter!r}')
        if label_filter is not None:
            _rank._need_labels(self.labels, self.local.shape[0], f'label_filter="{label_filter}"', _SHARD_LABELS)
            if query_labels is None:
                raise MI355Error(f'label_filter="{label_filter}" needs query_labels')

    def _exchange_queries(self, queries_local, query_labels=None, exclude=None, side: bool = True):
        """The ONE query exchange: (all world*Q_local queries rank-major, their labels or None, their exclude rows or None), the
        same on every rank.  The per-query side of a filter travels as one (Q_local, 2) int64 [label, exclude] tensor, -1 where
        not given: one all-gather for the queries and one for the side (``side=False``, the plain search: none for the side);
        no collective at world_size == 1."""
        q = queries_local.float().contiguous()
        Ql = q.shape[0]
        if side:
            alls = torch.full((Ql, 2), -1, dtype=torch.int64, device=self.device)
            for col, t, name in ((0, query_labels, "query_labels"), (1, exclude, "exclude")):
                if t is None:
                    continue
                if (not torch.is_tensor(t) or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool
                        or t.dim() != 1 or t.shape[0] != Ql):
                    raise MI355Error(f"{name} must be an integer tensor of shape ({Ql},)")
                if t.device != self.device:
                    raise MI355Error(f"{name} is on {t.device} but the shard on {self.device}")
                alls[:, col] = t
        allq = q
        if self.world > 1:
            dist = torch.distributed
            allq = torch.empty((self.world * Ql, self.dim), dtype=torch.float32, device=self.device)
            dist.all_gather_into_tensor(allq, q, group=self.group)
            if side:
                mine, alls = alls, torch.empty((self.world * Ql, 2), dtype=torch.int64, device=self.device)
                dist.all_gather_into_tensor(alls, mine, group=self.group)
        return (allq, alls[:, 0].contiguous() if side and query_labels is not None else None,
                alls[:, 1].contiguous() if side and exclude is not None else None)

    def _exchange_candidates(self, allq, k, idx_offset, shard_offsets, **filt):
        """The ONE candidate exchange: this shard's top-k of ``allq`` packed as (Q, k, 2) int32 {f32 score bits, row index +
        idx_offset} (a short or empty shard pads to exactly k slots with {-inf, -1}: mi355_pack_candidates), one all-gather of
        it (rank-major), then ``shard_offsets`` added and world * k candidates merged per query in one library call
        (mi355_merge_packed_topk: no torch elementwise kernels on the rank stream)."""
        Q = allq.shape[0]
        kk = min(k, self.local.shape[0])
        v, i = self.ops.local_topk(allq, self.shard, kk, idx_offset, **filt) if kk > 0 else (None, None)
        allp = self.ops.pack(v, i, Q, k, self.device)
        if self.world > 1:
            packed, allp = allp, torch.empty((self.world * Q, k, 2), dtype=torch.int32, device=self.device)
            torch.distributed.all_gather_into_tensor(allp, packed, group=self.group)
        return self.ops.merge_packed(allp.view(self.world, Q, k, 2), shard_offsets, k)

    def _expand_queries(self, q, n, alpha, query_labels, label_filter, exclude):
        """Alpha query expansion of this rank's queries against the WHOLE gallery, bit for bit that of one ``Gallery`` holding
        every row: round 1 is ``search(q, n)`` (merged global lists, the same on every rank); each rank writes the neighbour
        rows it owns into a (Q, n, D) fp32 slab that is +0.0 elsewhere, and ONE all_reduce(SUM) of the slab viewed as int32
        combines them exactly (one rank contributes each row's bits, -0.0 included); then every rank expands its own
        queries over its part of the slab (mi355_expand_rows, the exchanged rows as an fp32 gallery of Q * n rows)."""
        vals, idx = self.search(q, n, query_labels=query_labels, label_filter=label_filter, exclude=exclude)
        Q = idx.shape[0]
        slab = self.ops.qe_slab(idx, self.offset, self.local)
        if self.world > 1:
            torch.distributed.all_reduce(slab.view(torch.int32), op=torch.distributed.ReduceOp.SUM, group=self.group)
        Ql = q.shape[0]
        mine = slice(self.rank * Ql, (self.rank + 1) * Ql)
        pos = torch.arange(Ql * n, dtype=torch.int64, device=self.device).view(Ql, n)
        local_idx = torch.where(idx[mine] >= 0, pos, torch.full_like(pos, -1))
        return self.ops.expand(q, slab[mine].contiguous(), vals[mine].contiguous(), local_idx, alpha, _rank._EPS) if Q else q

    def search(self, queries_local: torch.Tensor, k: int, *, query_labels: torch.Tensor | None = None,
               label_filter: str | None = None, exclude: torch.Tensor | None = None, qe=None):
        """Top-k of every rank's queries against the WHOLE gallery.

        ``queries_local``: this rank's (Q_local, D) queries (same Q_local on every rank).
        Returns (values, global indices) for ALL world*Q_local queries, rank-major, on every rank.

        Filtered search (see ``cosine_topk``): ``label_filter`` "same" / "different" compares the shards' labels with this
        rank's ``query_labels`` (Q_local,); ``exclude`` (Q_local,) holds GLOBAL row indices.  Every shard searches with its
        own labels and its offset as idx_offset (so ``exclude`` compares global rows) and packs GLOBAL indices; the merge then
        adds zero offsets, and slots that no shard filled become (-inf, -1).

        ``qe=(n, alpha)``: alpha query expansion (``Gallery.search``'s ``qe``), the same filter arguments in both rounds; bit for
        bit the result of one ``Gallery`` holding every row.  (Database-side augmentation has no sharded form.)"""
        if k < 1 or k > self.total_rows:
            raise MI355Error(f"selected index k out of range: k={k}, gallery rows={self.total_rows}")
        self._check_filter(label_filter, query_labels)
        if qe is not None:
            n, alpha = _rank._qe_pair(qe)
            if n > self.total_rows:
                raise MI355Error(f"selected index k out of range: k={n}, gallery rows={self.total_rows}")
            filt = dict(query_labels=query_labels, label_filter=label_filter, exclude=exclude)
            q2 = self._expand_queries(queries_local.float().contiguous(), n, alpha, **filt)
            return self.search(q2, k, **filt)
        if label_filter is None and exclude is None:
            if self.world == 1:
                return self.ops.local_topk(queries_local.float().contiguous(), self.shard, k, 0)
            allq, _, _ = self._exchange_queries(queries_local, side=False)
            return self._exchange_candidates(allq, k, 0, self._offsets_dev)          # LOCAL indices + the shard offsets
        if self.total_rows >= 2 ** 31 - 128:
            raise MI355Error("a filtered sharded search carries global int32 indices: the gallery must have fewer than 2^31 rows")
        allq, ql, ex = self._exchange_queries(queries_local, query_labels if label_filter is not None else None, exclude)
        zeros = torch.zeros(self.world, dtype=torch.int64, device=self.device)
        vals, idx = self._exchange_candidates(allq, k, self.offset, zeros, query_labels=ql, gallery_labels=self.labels,
                                              label_filter=label_filter, exclude=ex)
        return self.ops.clear_pads(vals, idx, 0, self.total_rows)

    def range_search(self, queries_local: torch.Tensor, threshold: float, *, query_labels: torch.Tensor | None = None,
                     label_filter: str | None = None, exclude: torch.Tensor | None = None, max_results: int | None = None):
        """``cosine_range`` of every rank's queries against the WHOLE gallery: a ``RangeResult`` for all world*Q_local
        queries, rank-major, the same on every rank and bit for bit that of one gallery holding every row.

        The queries and their filter side (``query_labels`` / ``exclude`` (Q_local,), GLOBAL rows) are all-gathered as in
        ``search``; each rank searches its shard with its offset as idx_offset; the per-query hit counts are all-gathered,
        then the payloads padded to the largest shard's hit count.  A query's hits are its shards' hits in rank order (shard
        offsets ascend with rank: already ascending rows, no merge).  ``max_results`` applies to the whole result."""
        self._check_filter(label_filter, query_labels)
        if max_results is not None and int(max_results) < 0:
            raise MI355Error(f"max_results must be >= 0 or None, got {max_results}")
        threshold = _rank._range_threshold(threshold)
        allq, ql, ex = self._exchange_queries(queries_local, query_labels if label_filter is not None else None, exclude)
        Q = allq.shape[0]
        dist = torch.distributed
        if self.local.shape[0]:
            local = self.ops.local_range(allq, self.shard, threshold, self.offset, query_labels=ql, gallery_labels=self.labels,
                                         label_filter=label_filter, exclude=ex)
        else:
            local = _rank._range_empty(Q, self.device)
        counts = local.offsets[1:] - local.offsets[:-1]                                   # (Q,) hits per query in this shard
        if self.world == 1:
            if max_results is not None and local.indices.shape[0] > int(max_results):
                raise MI355Error(f"the range search has {local.indices.shape[0]} hits, more than max_results={int(max_results)}")
            return local
        allc = torch.empty(self.world * Q, dtype=torch.int64, device=self.device)
        dist.all_gather_into_tensor(allc, counts.contiguous(), group=self.group)
        allc = allc.view(self.world, Q)
        shard_nnz = allc.sum(1).cpu().tolist()                                             # the one host sync of the exchange
        total = sum(shard_nnz)
        if max_results is not None and total > int(max_results):
            raise MI355Error(f"the range search has {total} hits, more than max_results={int(max_results)}")
        pad = max(max(shard_nnz), 1)                                                       # (no empty collective)
        # payload: (pad, 2) int64 [global row, score bits]
        payload = torch.zeros((pad, 2), dtype=torch.int64, device=self.device)
        n = local.indices.shape[0]
        payload[:n, 0] = local.indices
        payload[:n, 1] = local.scores.view(torch.int32).to(torch.int64)
        allp = torch.empty((self.world * pad, 2), dtype=torch.int64, device=self.device)
        dist.all_gather_into_tensor(allp, payload, group=self.group)
        # segment (q, r) = shard r's hits of query q, taken in q-major, r-minor order
        seg_len = allc.t().reshape(-1)                                                     # (Q * world,)
        starts = torch.zeros((self.world, Q), dtype=torch.int64, device=self.device)
        starts[:, 1:] = allc[:, :-1].cumsum(1)
        src0 = (starts + torch.arange(self.world, dtype=torch.int64, device=self.device)[:, None] * pad).t().reshape(-1)
        dst0 = seg_len.cumsum(0) - seg_len
        pos = torch.arange(total, dtype=torch.int64, device=self.device)
        src = (torch.repeat_interleave(src0 - dst0, seg_len, output_size=total) + pos) if total else pos
        offsets = torch.zeros(Q + 1, dtype=torch.int64, device=self.device)
        offsets[1:] = allc.sum(0).cumsum(0)
        out = allp[src]
        return _rank.RangeResult(offsets, out[:, 0].contiguous(), out[:, 1].to(torch.int32).view(torch.float32).contiguous())

    def verification_roc(self, queries_local: torch.Tensor, query_labels_local: torch.Tensor, thresholds=None,
                         exclude: torch.Tensor | None = None):
        """``verification_roc`` of every rank's queries against the WHOLE gallery (the shard labels given to the constructor).

        ``queries_local`` (Q_local, D) and ``query_labels_local`` (Q_local,) of this rank (same Q_local on every rank);
        ``exclude`` (Q_local,) GLOBAL row indices (negative = none).  The queries, labels and exclude are all-gathered as
        ``search`` does, each rank counts its shard's pairs, and ONE all_reduce(SUM) of the int64 histogram gives every rank
        the same result, bit for bit that of one gallery holding every row."""
        gl = _rank._need_labels(self.labels, self.local.shape[0], "verification_roc", _SHARD_LABELS)
        allq, ql, ex = self._exchange_queries(queries_local, query_labels_local, exclude)
        thr = _rank._roc_thresholds(thresholds, self.device)
        hist = self.ops.roc_hist(allq, ql, self.shard, gl, ex, self.offset, thr)
        if self.world > 1:
            torch.distributed.all_reduce(hist, op=torch.distributed.ReduceOp.SUM, group=self.group)
        return self.ops.roc_finalize(hist, thr)

    def fit_whitening(self, dim_out: int | None = None, *, power: float = 0.5, ridge: float = 1e-5):
        """``Whitening`` fitted on the WHOLE gallery.  Moment sums are additive: each rank takes the float64 moments of its
        shard (an empty shard contributes zeros), ONE all_gather of the packed ``[n, sum, outer]`` vector (1 + D + D^2 float64
        per rank) brings them to every rank, they are added in rank order and ``Whitening.from_moments`` runs on every rank:
        all ranks hold the same bits.  world_size == 1 makes no collective call."""
        from .whitening import Whitening
        D = self.dim
        n_local = self.local.shape[0]
        packed = torch.zeros(1 + D + D * D, dtype=torch.float64, device=self.device)
        if n_local:
            s, o = self.ops.moments(self.shard)
            packed[0] = float(n_local)
            packed[1: 1 + D] = s.to(self.device, torch.float64)
            packed[1 + D:] = o.to(self.device, torch.float64).reshape(-1)
        if self.world > 1:
            flat = torch.empty(self.world * packed.numel(), dtype=torch.float64, device=self.device)    # rank-major concat
            torch.distributed.all_gather_into_tensor(flat, packed, group=self.group)
            allm = flat.view(self.world, packed.numel())
            total = allm[0].clone()
            for r in range(1, self.world):                        # rank order: the same sum on every rank
                total += allm[r]
        else:
            total = packed
        total = total.cpu()
        return Whitening.from_moments(int(total[0].item()), total[1: 1 + D].clone(), total[1 + D:].reshape(D, D).clone(), dim_out,
                                      power=power, ridge=ridge, normalize_input=True, device=self.device)

    def whitened(self, w) -> "ShardedGallery":
        """A new ``ShardedGallery`` (same group, labels and dtype; prepared as this one) over the whitening ``w`` of this
        rank's rows, fp32 or fp16 read where they lie (one ``mi355_whiten_rows`` launch)."""
        if self.dim != w.dim_in:
            raise MI355Error(f"the whitening takes {w.dim_in} columns but the gallery has {self.dim}")
        src = _rank._Rows.of(self.shard, True)
        rows = torch.empty((src.rows, w.dim_out), dtype=torch.float32, device=self.device)
        w._apply(src, False, rows, True)
        return ShardedGallery(rows, group=self.group, ops=self.ops, labels=self.labels, prepared=self.prepared is not None,
                              dtype=src.dtype)

    def my_slice(self, Q_local: int) -> slice:
        """Rows of ``search``'s result that belong to this rank's own queries."""
        return slice(self.rank * Q_local, (self.rank + 1) * Q_local)
