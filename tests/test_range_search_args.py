"""Cosine range search without a GPU: the new C symbols, every argument check of the new entries (each refused before any HIP
call, with a message), the Python-side checks that need no device tensor, and ShardedGallery.range_search's assembly (count
all-gather, padded payload all-gather, per-query concatenation in rank order) through an injected CPU backend under gloo."""
import ctypes as C
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib
from imageretrievalresearch_amd import rank as R
from imageretrievalresearch_amd.sharded import ShardedGallery

NEW = ["mi355_range_workspace_bytes", "mi355_cosine_range", "mi355_range_f16_workspace_bytes", "mi355_cosine_range_f16",
       "mi355_range_compact"]
FAKE = C.c_void_p(4096)          # never dereferenced: every call below fails its argument checks first


def test_new_symbols_are_declared_bound_and_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name
    import imageretrievalresearch_amd as M
    assert "cosine_range" in M.__all__ and M.cosine_range is R.cosine_range
    assert hasattr(R.Gallery, "range_search") and hasattr(ShardedGallery, "range_search")


def _nnz():
    return C.byref(C.c_int64(-1))


def _search(q=FAKE, g=FAKE, Q=8, G=100, dim=64, thr=0.5, filt=None, cand=FAKE, cap=16, nnz=True, ws=FAKE, wsb=1 << 40):
    return _lib.lib().mi355_cosine_range(q, Q, g, G, dim, 0, 1e-6, thr, 0, filt, cand, cap, _nnz() if nnz else None, ws, wsb, None)


def _search16(q=FAKE, g=FAKE, Q=8, G=100, dim=64, thr=0.5, filt=None, cand=FAKE, cap=16, nnz=True, ws=FAKE, wsb=1 << 40):
    return _lib.lib().mi355_cosine_range_f16(q, Q, g, G, dim, 1e-6, thr, 0, filt, cand, cap, _nnz() if nnz else None, ws, wsb, None)


@pytest.mark.parametrize("entry", [_search, _search16], ids=["fp32", "fp16"])
def test_search_entry_checks(entry):
    L = _lib.lib()
    bad_filter = _lib.RankFilter()
    bad_filter.label_mode = 1                      # "same" without labels
    odd_filter = _lib.RankFilter()
    odd_filter.label_mode = 7
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(q=None), b"null queries/gallery"),
        (dict(g=None), b"null queries/gallery"),
        (dict(nnz=False), b"null nnz"),
        (dict(Q=-1), b"bad shape"),
        (dict(G=-1), b"bad shape"),
        (dict(dim=0), b"bad shape"),
        (dict(G=1 << 31), b"shape too large"),
        (dict(thr=nan), b"threshold is not finite"),
        (dict(thr=inf), b"threshold is not finite"),
        (dict(thr=-inf), b"threshold is not finite"),
        (dict(cap=-1), b"capacity=-1"),
        (dict(cand=None), b"null candidates"),
        (dict(cand=C.c_void_p(4097)), b"8-byte aligned"),
        (dict(filt=C.byref(bad_filter)), b"needs query_labels and gallery_labels"),
        (dict(filt=C.byref(odd_filter)), b"unknown label_mode 7"),
        (dict(ws=None), b"workspace"),
        (dict(wsb=16), b"workspace"),
    ]
    for kw, msg in cases:
        assert entry(**kw) != 0, kw
        assert msg in L.mi355_last_error(), (kw, msg, L.mi355_last_error())
    assert _search16(g=C.c_void_p(4104)) != 0 and b"16-byte aligned" in L.mi355_last_error()


def test_compact_entry_checks():
    L = _lib.lib()

    def compact(cand=FAKE, cap=16, Q=8, nnz=4, ws=FAKE, wsb=1 << 20, off=FAKE, idx=FAKE, sc=FAKE):
        return L.mi355_range_compact(cand, cap, Q, nnz, 0, ws, wsb, off, idx, sc, None)

    cases = [
        (dict(Q=-1), b"Q=-1"),
        (dict(nnz=17), b"nnz=17 outside [0, capacity=16]"),
        (dict(nnz=-1), b"nnz=-1"),
        (dict(cand=None), b"null candidates"),
        (dict(off=None), b"null offsets"),
        (dict(idx=None), b"null indices/scores"),
        (dict(sc=None), b"null indices/scores"),
        (dict(ws=None), b"workspace"),
        (dict(Q=1 << 20, wsb=1024), b"workspace"),
    ]
    for kw, msg in cases:
        assert compact(**kw) != 0, kw
        assert msg in L.mi355_last_error(), (kw, msg, L.mi355_last_error())


def test_workspace_has_no_pair_term():
    L = _lib.lib()
    # normalised queries + one call's planes + 1 / |row| + the (query, tile) table of one query block: no Q x G term
    for fn in (L.mi355_range_workspace_bytes, L.mi355_range_f16_workspace_bytes):
        assert fn(100000, 100000, 1536) < 100000 * 1536 * 4 + 512 * 2**20
        assert fn(1000000, 1000000, 64) < 1000000 * 64 * 4 + 512 * 2**20
        assert fn(256, 100000, 1536) < 32 * 2**20
        assert fn(-1, 10, 8) == 0 and fn(4, 10, 0) == 0
        assert 0 < fn(0, 10, 8) < 4096 and 0 < fn(5, 0, 8) < 4096       # empty shapes: the offsets only


def test_python_side_errors_without_a_device():
    with pytest.raises(MI355Error, match="must live on the GPU"):
        R.cosine_range(torch.zeros(4, 8), torch.zeros(5, 8), 0.5)
    g = R.Gallery(8, "cpu")
    with pytest.raises(MI355Error, match="needs gallery labels"):
        g.range_search(torch.zeros(4, 8), 0.5, query_labels=torch.zeros(4, dtype=torch.int64), label_filter="same")
    with pytest.raises(MI355Error, match="threshold must be finite"):
        R._range_threshold(float("nan"))
    with pytest.raises(MI355Error, match="threshold must be finite"):
        R._range_threshold(float("-inf"))
    assert R._range_threshold(0.75) == 0.75


class _CpuOps:
    """An injected CPU backend: scores in float64 with a fixed summation order (the same bits for a pair wherever it sits),
    rounded to fp32, then the hits of each query in ascending row order, as the HIP entry returns them."""

    @staticmethod
    def normalize(rows):
        return rows / rows.norm(dim=1, keepdim=True).clamp_min(1e-6)

    @staticmethod
    def local_range(queries, gallery_normalized, threshold, idx_offset, gallery_f16=None, query_labels=None,
                    gallery_labels=None, label_filter=None, exclude=None):
        q = _CpuOps.normalize(queries.double())
        g = gallery_normalized.double()
        s = torch.zeros((q.shape[0], g.shape[0]), dtype=torch.float64)
        for d in range(q.shape[1]):
            s += q[:, d, None] * g[None, :, d]
        s = s.float()
        hit = s.double() >= threshold
        if label_filter is not None:
            same = query_labels[:, None] == gallery_labels[None, :]
            hit &= same if label_filter == "same" else ~same
        if exclude is not None:
            hit &= (torch.arange(g.shape[0])[None, :] + idx_offset) != exclude[:, None]
        qi, gi = hit.nonzero(as_tuple=True)
        offsets = torch.zeros(q.shape[0] + 1, dtype=torch.int64)
        offsets[1:] = hit.sum(1).cumsum(0)
        return R.RangeResult(offsets, gi + idx_offset, s[qi, gi])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(n_rows, world, Ql, D=16):
    gen = torch.Generator().manual_seed(7)
    G = torch.randn(n_rows, D, generator=gen)
    G[n_rows // 2] = G[1]                                    # a duplicate row in another shard
    Qall = torch.randn(world * Ql, D, generator=gen)
    Qall[0] = G[1]
    labels = torch.arange(n_rows) % 3
    qlab = torch.arange(world * Ql) % 3
    excl = torch.arange(world * Ql) * 7 % (n_rows + 3) - 2   # some negative (none), some past the gallery
    return G, Qall, labels, qlab, excl


def _worker(rank, world, port, bounds, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        Ql, t = 4, 0.1
        G, Qall, labels, qlab, excl = _data(bounds[-1], world, Ql)
        lo, hi = bounds[rank], bounds[rank + 1]
        gal = ShardedGallery(G[lo:hi].clone(), ops=_CpuOps, labels=labels[lo:hi].clone())
        mine = slice(rank * Ql, (rank + 1) * Ql)
        ok = True
        for kw, full_kw in (({}, {}),
                            (dict(query_labels=qlab[mine], label_filter="different", exclude=excl[mine]),
                             dict(query_labels=qlab, gallery_labels=labels, label_filter="different", exclude=excl)),
                            (dict(query_labels=qlab[mine], label_filter="same"),
                             dict(query_labels=qlab, gallery_labels=labels, label_filter="same"))):
            r = gal.range_search(Qall[mine].clone(), t, **kw)
            w = _CpuOps.local_range(Qall, _CpuOps.normalize(G), t, 0, **full_kw)
            ok = ok and torch.equal(r.offsets, w.offsets) and torch.equal(r.indices, w.indices)
            ok = ok and torch.equal(r.scores.view(torch.int32), w.scores.view(torch.int32))
            ok = ok and int(w.offsets[-1]) > 0
        # max_results applies to the whole result, on every rank alike
        total = int(_CpuOps.local_range(Qall, _CpuOps.normalize(G), t, 0).offsets[-1])
        try:
            gal.range_search(Qall[mine].clone(), t, max_results=total - 1)
            ok = False
        except MI355Error:
            pass
        ok = ok and int(gal.range_search(Qall[mine].clone(), t, max_results=total).offsets[-1]) == total
        # a threshold nothing reaches: an empty result with zero offsets
        e = gal.range_search(Qall[mine].clone(), 1.5)
        ok = ok and e.indices.numel() == 0 and not bool(e.offsets.any()) and e.offsets.shape == (world * Ql + 1,)
        out[rank] = bool(ok)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world,bounds", [(2, [0, 40, 90]), (3, [0, 31, 31, 80]), (3, [0, 1, 50, 51])],
                         ids=["world2", "world3-empty-shard", "world3-ragged"])
def test_sharded_range_equals_unsharded(world, bounds):
    port = _free_port()
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, bounds, out), nprocs=world, join=True)
    assert all(out.get(r) for r in range(world)), dict(out)


def test_sharded_range_world_one_and_checks():
    G, Qall, labels, qlab, excl = _data(30, 1, 5)
    gal = ShardedGallery(G, ops=_CpuOps, labels=labels)
    r = gal.range_search(Qall, 0.2, exclude=excl)
    w = _CpuOps.local_range(Qall, _CpuOps.normalize(G), 0.2, 0, exclude=excl)
    assert torch.equal(r.offsets, w.offsets) and torch.equal(r.indices, w.indices) and torch.equal(r.scores, w.scores)
    with pytest.raises(MI355Error, match="threshold must be finite"):
        gal.range_search(Qall, float("nan"))
    with pytest.raises(MI355Error, match="needs query_labels"):
        gal.range_search(Qall, 0.2, label_filter="same")
    with pytest.raises(MI355Error, match="label_filter must be"):
        gal.range_search(Qall, 0.2, label_filter="other")
    with pytest.raises(MI355Error, match="exclude must be an integer tensor"):
        gal.range_search(Qall, 0.2, exclude=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(MI355Error, match="needs the shard labels"):
        ShardedGallery(G, ops=_CpuOps).range_search(Qall, 0.2, query_labels=qlab, label_filter="different")
    with pytest.raises(MI355Error, match="max_results"):
        gal.range_search(Qall, 0.2, max_results=0)
