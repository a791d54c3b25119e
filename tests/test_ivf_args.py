"""The IVF entries without a GPU: the ABI names, every argument error of mi355_ivf_scan before any HIP call, its workspace
sizer, the Python argument checks of ivf.py, and the float64 reference against a brute-force loop."""
import ctypes

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import ivf_ref as ref
from helpers import header_symbols
from imageretrievalresearch_amd import _lib, ivf

NEW = ["mi355_ivf_scan", "mi355_ivf_scan_workspace_bytes"]
P = 0x1000        # a non-null, 16-byte aligned address that no check may dereference


def test_new_entries_are_declared_bound_and_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name
    assert _lib.lib().mi355_abi_version() == 3
    assert M.IVFIndex is ivf.IVFIndex and "IVFIndex" in M.__all__ and hasattr(M.Gallery, "ivf")


def _fails(status, word):
    msg = _lib.lib().mi355_last_error()
    assert status != 0 and word.encode() in msg, (status, msg)


def _scan(q=P, Q=3, dim=8, rows=P, dtype=_lib.DTYPE_F32, ld=8, G=100, off=P, order=P, nlist=10, probes=P, nprobe=2, cap=50,
          filt=None, cv=P, ci=P, ws=P, wsb=1 << 30):
    return _lib.lib().mi355_ivf_scan(q, Q, dim, 1e-6, rows, dtype, ld, G, off, order, nlist, probes, nprobe, cap, 0, filt, cv, ci,
                                     ws, wsb, None)


def test_scan_argument_errors():
    for kw in ("q", "rows", "off", "order", "probes", "cv", "ci"):
        _fails(_scan(**{kw: None}), "null")
    _fails(_scan(Q=-1), "Q=")
    _fails(_scan(dtype=2), "dtype")
    _fails(_scan(dtype=-1), "dtype")
    _fails(_scan(dim=0), "dim=")
    _fails(_scan(G=0), "G=")
    _fails(_scan(ld=7), "ld=")
    _fails(_scan(nlist=0), "nlist")
    _fails(_scan(nlist=1 << 24, nprobe=1), "nlist")
    _fails(_scan(nprobe=0), "nprobe")
    _fails(_scan(nprobe=11), "nprobe")
    _fails(_scan(cap=0), "cap=")
    _fails(_scan(Q=1 << 30, nprobe=2), "too large")                       # Q * nprobe >= 2^31
    _fails(_scan(Q=1 << 20, cap=(1 << 20) + 1), "too large")              # Q * cap > 2^40
    _fails(_scan(dim=16388, ld=16388), "LDS")                             # one fp32 query no longer fits in 64 KB
    _fails(_scan(dim=16384, ld=16384, ws=None, wsb=0), "workspace")       # ... and the largest one that does
    _fails(_scan(dtype=_lib.DTYPE_F16, rows=P + 2, ld=64), "16-byte aligned")
    _fails(_scan(dtype=_lib.DTYPE_F16, ld=12), "multiple of 8")
    _fails(_scan(ws=None, wsb=0), "workspace")
    _fails(_scan(wsb=64), "workspace")
    f = _lib.RankFilter()
    f.label_mode = 7
    _fails(_scan(filt=ctypes.byref(f)), "label_mode")
    f.label_mode = _lib.LABEL_SAME
    _fails(_scan(filt=ctypes.byref(f)), "needs query_labels")
    # no query: nothing to do, whatever the pointers (but the scalar arguments are still checked)
    assert _scan(Q=0, q=None, cv=None, ci=None, ws=None, wsb=0) == 0
    _fails(_scan(Q=0, nprobe=0), "nprobe")


def test_workspace_rises_with_the_queries_and_the_probes():
    ws = _lib.lib().mi355_ivf_scan_workspace_bytes
    assert ws(0, 2, 10, 8, 50) == 0 and ws(3, 0, 10, 8, 50) == 0 and ws(3, 11, 10, 8, 50) == 0 and ws(3, 2, 0, 8, 50) == 0
    assert ws(3, 2, 10, 0, 50) == 0 and ws(3, 2, 10, 8, 0) == 0
    last = 0
    for Q in (1, 2, 5, 64, 65, 256, 257, 4096):
        now = ws(Q, 16, 1024, 1536, 40000)
        assert now > last, (Q, now, last)
        last = now
    last = 0
    for nprobe in (1, 2, 3, 8, 32, 33, 1024):
        now = ws(256, nprobe, 1024, 1536, 40000)
        assert now > last, (nprobe, now, last)
        last = now
    # the queries, three int64 per pair, the item table (16 B per 64 candidate slots and per pair) and the small tables
    assert ws(256, 16, 1024, 1536, 40000) < 256 * 1536 * 4 + 256 * 16 * (24 + 16 + 8) + 256 * 40000 // 4 + (1 << 16)


def _fake_index(rows=500, nlist=9, gallery_rows=None):
    ix = ivf.IVFIndex.__new__(ivf.IVFIndex)
    g = M.Gallery.__new__(M.Gallery)
    g.rows, g.dim, g.labels = rows if gallery_rows is None else gallery_rows, 4, None
    ix.gallery, ix.rows, ix.nlist = g, rows, nlist
    ix._longest = np.arange(nlist + 1) * 10
    return ix


def test_python_argument_checks_come_before_any_launch(monkeypatch):
    monkeypatch.setattr(ivf, "lib", lambda: pytest.fail("reached the library"))
    ix = _fake_index()
    q = torch.zeros(3, 4)
    pr = torch.zeros(3, 2, dtype=torch.int64)
    for k in (0, -1, 501, 2.0, True, None):
        with pytest.raises(M.MI355Error, match="k out of range"):
            ix.search(q, k, nprobe=1)
    with pytest.raises(M.MI355Error, match="k out of range"):
        _fake_index(rows=5000).search(q, 1025, nprobe=1)
    with pytest.raises(M.MI355Error, match="exactly one"):
        ix.search(q, 3)
    with pytest.raises(M.MI355Error, match="exactly one"):
        ix.search(q, 3, nprobe=2, probes=pr)
    for nprobe in (0, -1, 10, 1.0, True):
        with pytest.raises(M.MI355Error, match="nprobe"):
            ix.search(q, 3, nprobe=nprobe)
        with pytest.raises(M.MI355Error, match="nprobe"):
            ix.probe(q, nprobe)
    with pytest.raises(M.MI355Error, match="nprobe"):
        _fake_index(nlist=2000, rows=5000).search(q, 3, nprobe=1025)
    with pytest.raises(M.MI355Error, match="stale"):
        _fake_index(gallery_rows=501).search(q, 3, nprobe=1)
    with pytest.raises(M.MI355Error, match="GPU"):                         # host tensors: no CPU path
        ix.search(q, 3, nprobe=1)
    with pytest.raises(M.MI355Error, match="GPU"):
        ix.search(q, 3, probes=pr)
    with pytest.raises(M.MI355Error, match="Gallery"):
        M.IVFIndex(torch.zeros(4, 4), torch.zeros(2, 4), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="Gallery"):
        M.IVFIndex.build(torch.zeros(4, 4), 2)
    empty = M.Gallery.__new__(M.Gallery)
    empty.rows = 0
    with pytest.raises(M.MI355Error, match="at least one row"):
        M.IVFIndex(empty, torch.zeros(2, 4), torch.zeros(0, dtype=torch.int64))


def test_shape_checks_of_search(monkeypatch):
    # pretend the tensors are on the GPU: the shapes must be refused before the library is reached
    from imageretrievalresearch_amd import rank
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)
    monkeypatch.setattr(ivf, "lib", lambda: pytest.fail("reached the library"))
    ix = _fake_index()
    g = ix.gallery
    g._buf, g.device, g.dtype, g._prepared, g._prepared_rows, g.eps = torch.zeros(500, 4), torch.device("cpu"), torch.float32, None, 0, 1e-6
    q = torch.zeros(3, 4)
    with pytest.raises(M.MI355Error, match="dims differ"):
        ix.search(torch.zeros(3, 5), 3, nprobe=1)
    with pytest.raises(M.MI355Error, match="probes must be"):
        ix.search(q, 3, probes=torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="probes must be"):
        ix.search(q, 3, probes=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="nprobe"):
        ix.search(q, 3, probes=torch.zeros(3, 10, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="integers"):
        ix.search(q, 3, probes=torch.zeros(3, 2))
    with pytest.raises(M.MI355Error, match="label_filter"):
        ix.search(q, 3, probes=torch.zeros(3, 2, dtype=torch.int64), label_filter="other")
    with pytest.raises(M.MI355Error, match="labels"):
        ix.search(q, 3, probes=torch.zeros(3, 2, dtype=torch.int64), label_filter="same", query_labels=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="exclude"):
        ix.search(q, 3, probes=torch.zeros(3, 2, dtype=torch.int64), exclude=torch.zeros(2, dtype=torch.int64))
    for block in (0, -2, 1.5, True):
        with pytest.raises(M.MI355Error, match="block"):
            ix.search(q, 3, probes=torch.zeros(3, 2, dtype=torch.int64), block=block)


def test_reference_against_a_brute_force_loop():
    rng = np.random.default_rng(0)
    G, D, Q, nlist = 40, 5, 6, 4
    rows = ref.normalise(rng.standard_normal((G, D)))
    x = rng.standard_normal((Q, D))
    assign = rng.integers(0, nlist - 1, G)                                  # the last list stays empty
    offsets, order = ref.lists_of(assign, nlist)
    assert offsets[-1] == G and offsets[-2] == G and sorted(order.tolist()) == list(range(G))
    for l in range(nlist):
        assert (order[offsets[l]: offsets[l + 1]] == np.nonzero(assign == l)[0]).all()
    probes = np.array([[0, 1], [1, 0], [3, 2], [2, 3], [0, 2], [3, 0]])
    glab, qlab, ex = rng.integers(0, 2, G), rng.integers(0, 2, Q), np.array([0, 1, 2, -1, 4, 5]) + 100
    S = ref.restricted_scores(rows, x, offsets, order, probes, query_labels=qlab, gallery_labels=glab, label_filter="different",
                              exclude=ex, idx_offset=100)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    for q in range(Q):
        for r in range(G):
            on = assign[r] in probes[q] and glab[r] != qlab[q] and r + 100 != ex[q]
            assert S[q, r] == (xn[q] @ rows[r] if on else -np.inf) or abs(S[q, r] - xn[q] @ rows[r]) < 1e-15
    v, i, gap = ref.topk(S, 30, idx_offset=100)
    for q in range(Q):
        fin = np.isfinite(S[q])
        n = int(fin.sum())
        assert n < 30 and (i[q, n:] == -1).all() and np.isneginf(v[q, n:]).all()
        assert sorted((i[q, :n] - 100).tolist()) == np.nonzero(fin)[0].tolist() and (np.diff(v[q, :n]) <= 0).all()
    assert ref.probed_rows(offsets, order, [2, 0]).tolist() == np.nonzero(assign == 2)[0].tolist() + np.nonzero(assign == 0)[0].tolist()
    tie = np.array([[1.0, 2.0, 2.0, -np.inf]])
    assert ref.topk(tie, 3)[1].tolist() == [[1, 2, 0]] and ref.topk(tie, 4)[1].tolist() == [[1, 2, 0, -1]] and ref.topk(tie, 2)[2][0] == 0.0
