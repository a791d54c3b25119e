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
"""
from __future__ import annotations

import torch

from . import rank as _rank
from ._lib import MI355Error



class _HipOps:
    """Default compute backend: the HIP library.  (Tests inject a CPU backend to exercise the
    collective plumbing under gloo without a GPU; the product path is always this one.)"""

    @staticmethod
    def local_topk(queries, gallery_normalized, k, idx_offset, prepared=None, **filt):
        # filt (filtered searches only): query_labels, gallery_labels, label_filter, exclude - the prepared planes have no
        # filtered search, the fp32 rows give the same results
        if not filt and prepared is not None and _rank.PreparedGallery.supports(queries.shape[0], k):
            return prepared.search(queries, k, idx_offset=idx_offset)
        return _rank.cosine_topk(queries, gallery_normalized, k, gallery_is_normalized=True, idx_offset=idx_offset, **filt)

    @staticmethod
    def roc_hist(queries, query_labels, gallery_normalized, gallery_labels, exclude, idx_offset, thr, gallery_f16=None):
        """The (2, T + 1) int64 pair histogram of ``queries`` against this shard (rows [idx_offset, ...) of the gallery)."""
        if gallery_f16 is not None:
            return gallery_f16._roc_hist(queries, query_labels, thr, exclude, idx_offset)
        ql = _rank._int64_on(query_labels, "query_labels", queries.shape[0], queries.device)
        gl = _rank._int64_on(gallery_labels, "gallery_labels", gallery_normalized.shape[0], queries.device)
        ex = None if exclude is None else _rank._int64_on(exclude, "exclude", queries.shape[0], queries.device)
        return _rank._roc_pairs_hist(queries, ql, gallery_normalized, gallery_normalized.shape[0], gl, ex, idx_offset, thr,
                                     gallery_is_normalized=True)

    @staticmethod
    def local_range(queries, gallery_normalized, threshold, idx_offset, gallery_f16=None, **filt):
        """``cosine_range`` of ``queries`` against this shard (rows [idx_offset, ...) of the gallery): a ``RangeResult`` with
        GLOBAL indices.  filt: query_labels, gallery_labels, label_filter, exclude."""
        if gallery_f16 is not None:
            filt.pop("gallery_labels", None)
            return gallery_f16.range_search(queries, threshold, idx_offset=idx_offset, **filt)
        return _rank.cosine_range(queries, gallery_normalized, threshold, gallery_is_normalized=True, idx_offset=idx_offset, **filt)

    @staticmethod
    def roc_finalize(hist, thr):
        return _rank._roc_finalize(hist, thr)

    @staticmethod
    def clear_pads(vals, idx, lo, hi):
        return _rank.clear_pads(vals, idx, lo, hi)

    @staticmethod
    def prepare(gallery_normalized):
        return _rank.PreparedGallery(gallery_normalized) if gallery_normalized.shape[0] else None

    @staticmethod
    def gallery_f16(local_rows):
        return _rank.Gallery(local_rows.shape[1], local_rows.device, capacity=local_rows.shape[0],
                             dtype=torch.float16).add(local_rows)

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
    def moments(local_rows, gallery_f16=None):
        """(sum (D,), outer (D, D)) float64 device tensors of this shard's normalised rows (mi355_embedding_moments)."""
        from .whitening import embedding_moments
        m = embedding_moments(gallery_f16 if gallery_f16 is not None else local_rows)
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
        # dtype=torch.float16: the shard is kept as an fp16 Gallery (half the bytes) and searched with its kernel
        self.gallery_f16 = self.ops.gallery_f16(local_rows.float().contiguous()) if dtype == torch.float16 else None
        if self.gallery_f16 is not None:
            self.local = self.gallery_f16.data
        else:
            self.local = self.ops.normalize(local_rows.float().contiguous()) if local_rows.shape[0] else local_rows.float()
        self.labels = labels
        if self.gallery_f16 is not None and labels is not None:
            self.gallery_f16.labels = labels.to(self.device, torch.int64)
        # prepared=True: the shard is also kept as the cosine GEMM's bf16 planes (+6 B per element; same results bit for bit)
        self.prepared = self.ops.prepare(self.local) if (prepared and hasattr(self.ops, "prepare")) else None
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

    def _local_topk(self, queries, k):
        if self.gallery_f16 is not None:
            return self.gallery_f16.search(queries, k)
        planes = {} if self.prepared is None else {"prepared": self.prepared}   # (an injected ops may take no prepared=)
        return self.ops.local_topk(queries, self.local, k, 0, **planes)

    def _local_candidates(self, queries, k):
        """(Q, k, 2) int32: [..., 0] = the f32 score's bits, [..., 1] = LOCAL row index; a short (or empty) shard pads to
        exactly k slots with {-inf, -1} (one library kernel: mi355_pack_candidates)."""
        Q = queries.shape[0]
        kk = min(k, self.local.shape[0])
        v, i = self._local_topk(queries, kk) if kk > 0 else (None, None)
        return self.ops.pack(v, i, Q, k, self.device)

    def _filtered_search(self, q, k, query_labels, label_filter, exclude):
        """Filtered search: every shard searches with its own labels and its offset as idx_offset (so ``exclude`` compares
        global rows) and packs GLOBAL indices; the merge then adds zero offsets, and slots that no shard filled become
        (-inf, -1)."""
        if label_filter is not None and self.labels is None:
            raise MI355Error(f'label_filter="{label_filter}" needs the shard labels: ShardedGallery(..., labels=)')
        if self.total_rows >= 2 ** 31 - 128:
            raise MI355Error("a filtered sharded search carries global int32 indices: the gallery must have fewer than 2^31 rows")
        Ql = q.shape[0]
        n_local = self.local.shape[0]
        if self.labels is not None and label_filter is not None and self.labels.shape[0] != n_local:
            raise MI355Error(f"the shard holds {self.labels.shape[0]} labels for {n_local} rows")
        # per-query side of the filter: (Ql, 2) int64 [label, exclude], all-gathered with ONE collective
        side = torch.full((Ql, 2), -1, dtype=torch.int64, device=self.device)
        if label_filter is not None:
            if query_labels is None:
                raise MI355Error(f'label_filter="{label_filter}" needs query_labels')
            side[:, 0] = _rank._int64_on(query_labels, "query_labels", Ql, self.device)
        if exclude is not None:
            side[:, 1] = _rank._int64_on(exclude, "exclude", Ql, self.device)
        dist = torch.distributed
        if self.world > 1:
            allq = torch.empty((self.world * Ql, self.dim), dtype=torch.float32, device=self.device)
            dist.all_gather_into_tensor(allq, q, group=self.group)
            alls = torch.empty((self.world * Ql, 2), dtype=torch.int64, device=self.device)
            dist.all_gather_into_tensor(alls, side, group=self.group)
        else:
            allq, alls = q, side
        Q = allq.shape[0]
        filt = {"label_filter": label_filter}
        if label_filter is not None:
            filt.update(query_labels=alls[:, 0].contiguous(), gallery_labels=self.labels)
        if exclude is not None:
            filt["exclude"] = alls[:, 1].contiguous()
        kk = min(k, n_local)
        if kk > 0:
            if self.gallery_f16 is not None:
                v, i = self.gallery_f16.search(allq, kk, self.offset, query_labels=filt.get("query_labels"),
                                               label_filter=label_filter, exclude=filt.get("exclude"))
            else:
                v, i = self.ops.local_topk(allq, self.local, kk, self.offset, **filt)
        else:
            v = i = None
        packed = self.ops.pack(v, i, Q, k, self.device)
        if self.world > 1:
            allp = torch.empty((self.world * Q, k, 2), dtype=torch.int32, device=self.device)
            dist.all_gather_into_tensor(allp, packed, group=self.group)
        else:
            allp = packed
        zeros = torch.zeros(self.world, dtype=torch.int64, device=self.device)
        vals, idx = self.ops.merge_packed(allp.view(self.world, Q, k, 2), zeros, k)
        return self.ops.clear_pads(vals, idx, 0, self.total_rows)

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
        rank's ``query_labels`` (Q_local,); ``exclude`` (Q_local,) holds GLOBAL row indices.  Slots no shard could fill are
        (-inf, -1).

        ``qe=(n, alpha)``: alpha query expansion (``Gallery.search``'s ``qe``), the same filter arguments in both rounds; bit for
        bit the result of one ``Gallery`` holding every row.  (Database-side augmentation has no sharded form.)"""
        if k < 1 or k > self.total_rows:
            raise MI355Error(f"selected index k out of range: k={k}, gallery rows={self.total_rows}")
        if label_filter not in (None, "same", "different"):
            raise MI355Error(f'label_filter must be None, "same" or "different", got {label_filter!r}')
        if qe is not None:
            n, alpha = _rank._qe_pair(qe)
            if n > self.total_rows:
                raise MI355Error(f"selected index k out of range: k={n}, gallery rows={self.total_rows}")
            filt = dict(query_labels=query_labels, label_filter=label_filter, exclude=exclude)
            q2 = self._expand_queries(queries_local.float().contiguous(), n, alpha, **filt)
            return self.search(q2, k, **filt)
        q = queries_local.float().contiguous()
        if label_filter is not None or exclude is not None:
            return self._filtered_search(q, k, query_labels, label_filter, exclude)
        if self.world == 1:
            return self._local_topk(q, k)
        dist = torch.distributed
        Ql = q.shape[0]
        allq = torch.empty((self.world * Ql, self.dim), dtype=torch.float32, device=self.device)
        dist.all_gather_into_tensor(allq, q, group=self.group)
        packed = self._local_candidates(allq, k)
        Q = allq.shape[0]
        allp = torch.empty((self.world * Q, k, 2), dtype=torch.int32, device=self.device)   # rank-major concat
        dist.all_gather_into_tensor(allp, packed, group=self.group)                             # the ONE candidate exchange
        # unpacking, the shard offsets and the merge of world * k candidates per query: one library call
        # (mi355_merge_packed_topk), no torch elementwise kernels on the rank stream
        return self.ops.merge_packed(allp.view(self.world, Q, k, 2), self._offsets_dev, k)

    def range_search(self, queries_local: torch.Tensor, threshold: float, *, query_labels: torch.Tensor | None = None,
                     label_filter: str | None = None, exclude: torch.Tensor | None = None, max_results: int | None = None):
        """``cosine_range`` of every rank's queries against the WHOLE gallery: a ``RangeResult`` for all world*Q_local
        queries, rank-major, the same on every rank and bit for bit that of one gallery holding every row.

        The queries and their filter side (``query_labels`` / ``exclude`` (Q_local,), GLOBAL rows) are all-gathered as in
        ``search``; each rank searches its shard with its offset as idx_offset; the per-query hit counts are all-gathered,
        then the payloads padded to the largest shard's hit count.  A query's hits are its shards' hits in rank order (shard
        offsets ascend with rank: already ascending rows, no merge).  ``max_results`` applies to the whole result."""
        if label_filter not in (None, "same", "different"):
            raise MI355Error(f'label_filter must be None, "same" or "different", got {label_filter!r}')
        if label_filter is not None and self.labels is None:
            raise MI355Error(f'label_filter="{label_filter}" needs the shard labels: ShardedGallery(..., labels=)')
        n_local = self.local.shape[0]
        if self.labels is not None and label_filter is not None and self.labels.shape[0] != n_local:
            raise MI355Error(f"the shard holds {self.labels.shape[0]} labels for {n_local} rows")
        if max_results is not None and int(max_results) < 0:
            raise MI355Error(f"max_results must be >= 0 or None, got {max_results}")
        threshold = _rank._range_threshold(threshold)
        q = queries_local.float().contiguous()
        Ql = q.shape[0]
        if label_filter is not None and query_labels is None:
            raise MI355Error(f'label_filter="{label_filter}" needs query_labels')
        side = torch.full((Ql, 2), -1, dtype=torch.int64, device=self.device)
        for col, t, name in ((0, query_labels if label_filter is not None else None, "query_labels"), (1, exclude, "exclude")):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype.is_floating_point or t.dtype == torch.bool or t.dim() != 1 or t.shape[0] != Ql:
                raise MI355Error(f"{name} must be an integer tensor of shape ({Ql},)")
            side[:, col] = t.to(self.device, torch.int64)
        dist = torch.distributed
        if self.world > 1:
            allq = torch.empty((self.world * Ql, self.dim), dtype=torch.float32, device=self.device)
            dist.all_gather_into_tensor(allq, q, group=self.group)
            alls = torch.empty((self.world * Ql, 2), dtype=torch.int64, device=self.device)
            dist.all_gather_into_tensor(alls, side, group=self.group)
        else:
            allq, alls = q, side
        Q = allq.shape[0]
        filt = {"label_filter": label_filter}
        if label_filter is not None:
            filt.update(query_labels=alls[:, 0].contiguous(), gallery_labels=self.labels)
        if exclude is not None:
            filt["exclude"] = alls[:, 1].contiguous()
        if n_local:
            local = self.ops.local_range(allq, self.local, threshold, self.offset, gallery_f16=self.gallery_f16, **filt)
        else:
            local = _rank.RangeResult(torch.zeros(Q + 1, dtype=torch.int64, device=self.device),
                                      torch.empty(0, dtype=torch.int64, device=self.device),
                                      torch.empty(0, dtype=torch.float32, device=self.device))
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
        if self.labels is None:
            raise MI355Error("verification_roc needs the shard labels: ShardedGallery(..., labels=)")
        n_local = self.local.shape[0]
        if self.labels.shape[0] != n_local:
            raise MI355Error(f"the shard holds {self.labels.shape[0]} labels for {n_local} rows")
        q = queries_local.float().contiguous()
        Ql = q.shape[0]
        side = torch.full((Ql, 2), -1, dtype=torch.int64, device=self.device)
        for col, t, name in ((0, query_labels_local, "query_labels"), (1, exclude, "exclude")):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype.is_floating_point or t.dim() != 1 or t.shape[0] != Ql:
                raise MI355Error(f"{name} must be an integer tensor of shape ({Ql},)")
            side[:, col] = t.to(self.device, torch.int64)
        thr = _rank._roc_thresholds(thresholds, self.device)
        dist = torch.distributed
        if self.world > 1:
            allq = torch.empty((self.world * Ql, self.dim), dtype=torch.float32, device=self.device)
            dist.all_gather_into_tensor(allq, q, group=self.group)
            alls = torch.empty((self.world * Ql, 2), dtype=torch.int64, device=self.device)
            dist.all_gather_into_tensor(alls, side, group=self.group)
        else:
            allq, alls = q, side
        ex = alls[:, 1].contiguous() if exclude is not None else None
        hist = self.ops.roc_hist(allq, alls[:, 0].contiguous(), self.local, self.labels, ex, self.offset, thr,
                                 gallery_f16=self.gallery_f16)
        if self.world > 1:
            dist.all_reduce(hist, op=dist.ReduceOp.SUM, group=self.group)
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
            s, o = self.ops.moments(self.local, gallery_f16=self.gallery_f16)
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
        rank's rows (``Gallery.whitened`` of the shard)."""
        if self.dim != w.dim_in:
            raise MI355Error(f"the whitening takes {w.dim_in} columns but the gallery has {self.dim}")
        if self.gallery_f16 is not None:
            rows = self.gallery_f16.whitened(w, dtype=torch.float32).data
            dtype = torch.float16
        else:
            rows = torch.empty((self.local.shape[0], w.dim_out), dtype=torch.float32, device=self.device)
            src = self.local.contiguous()
            w._apply(src, _rank._DTYPES[torch.float32], src.shape[0], self.dim, False, rows, True)
            dtype = torch.float32
        return ShardedGallery(rows, group=self.group, ops=self.ops, labels=self.labels, prepared=self.prepared is not None,
                              dtype=dtype)

    def my_slice(self, Q_local: int) -> slice:
        """Rows of ``search``'s result that belong to this rank's own queries."""
        return slice(self.rank * Q_local, (self.rank + 1) * Q_local)
