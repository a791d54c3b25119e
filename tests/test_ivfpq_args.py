"""IVF-PQ search, the parts that need no GPU: the C-ABI symbols, every argument check of the new entry (rejected before any HIP
call, with a message), the workspace sizes, the Python-side checks and the export."""
import ctypes

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, MI355Error, _lib, ivfpq, pq

NEW = ["mi355_ivfpq_search_workspace_bytes", "mi355_ivfpq_search"]
BIG = 1 << 40


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_declared_bound_and_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert L.mi355_abi_version() == 3
    assert ivfpq.SCAN_CHUNK == 2048


def test_workspace_sizes():
    s = _lib.lib().mi355_ivfpq_search_workspace_bytes          # (Q, nprobe, nlist, dim, M, cap, k)
    assert s(0, 8, 256, 1536, 96, 5000, 3) == 0                                       # Q = 0
    for k in (3, 150):                                                                # monotone in Q, cap and M
        assert 0 < s(1, 8, 256, 1536, 48, 5000, k) <= s(16, 8, 256, 1536, 48, 5000, k) <= s(256, 8, 256, 1536, 48, 5000, k) \
            <= s(1000, 8, 256, 1536, 48, 5000, k)
        assert s(16, 8, 256, 1536, 48, 1000, k) <= s(16, 8, 256, 1536, 48, 5000, k) <= s(16, 8, 256, 1536, 48, 100000, k)
        assert s(16, 8, 256, 1536, 48, 5000, k) <= s(16, 8, 256, 1536, 96, 5000, k)
    assert s(256, 32, 1024, 1536, 96, 100000, 3) < 64 << 20                           # k <= 8: tables and candidates, no slab
    assert s(256, 32, 1024, 1536, 96, 100000, 8) < 64 << 20
    assert s(256, 32, 1024, 1536, 96, 100000, 150) > 256 * 100000 * 12                # the (value, index) slab
    assert s(256, 32, 1024, 1536, 96, 100000, 3) >= 256 * 96 * 1024                   # the tables of a query block
    assert s(256, 32, 1024, 1536, 96, 10 ** 7, 150) < 2 << 30                         # the query block shrinks with the slab
    for bad in ((4, 8, 256, 64, 6, 100, 1), (4, 8, 256, 64, 132, 100, 1), (4, 8, 256, 66, 8, 100, 1), (4, 8, 256, 1024, 8, 100, 1),
                (4, 0, 256, 64, 8, 100, 1), (4, 257, 256, 64, 8, 100, 1), (4, 1025, 4096, 64, 8, 100, 1), (4, 8, 0, 64, 8, 100, 1),
                (4, 8, 1 << 24, 64, 8, 100, 1), (4, 8, 256, 64, 8, 0, 1), (4, 8, 256, 64, 8, 100, 0), (4, 8, 256, 64, 8, 100, 101),
                (4, 8, 256, 64, 8, 5000, 1025), (1 << 29, 8, 256, 64, 8, 100, 1), (1 << 20, 1, 256, 64, 8, 1 << 21, 1),
                (-1, 8, 256, 64, 8, 100, 1), (4, 8, 256, 0, 8, 100, 1)):
        assert s(*bad) == 0, bad


def test_search_argument_errors():
    L = _lib.lib()
    filt = _lib.RankFilter()

    def call(q=4096, Q=8, dim=64, cb=8192, M=8, codes=16384, G=1000, offsets=20480, order=24576, nlist=16, probes=28672, nprobe=4,
             cap=500, k=3, f=None, out=32768, out_idx=49152, ws=65536, ws_bytes=BIG):
        return L.mi355_ivfpq_search(q, Q, dim, 1e-6, cb, M, codes, G, offsets, order, nlist, probes, nprobe, cap, k, 0, f, out,
                                    out_idx, ws, ws_bytes, None)

    for name in ("q", "cb", "codes", "offsets", "order", "probes", "out", "out_idx"):
        assert call(**{name: None}) != 0 and b"null" in _err(), name
    assert call(Q=-1) != 0 and b"bad shape" in _err()
    assert call(G=0) != 0 and b"bad shape" in _err()
    assert call(M=6) != 0 and b"multiple of 4" in _err()                              # the PQ shape rules
    assert call(M=0) != 0 and b"multiple of 4" in _err()
    assert call(M=132, dim=132 * 4) != 0 and b"multiple of 4 in [4, 128]" in _err()
    assert call(dim=66) != 0 and b"multiple of M" in _err()
    assert call(dim=0) != 0 and _err()
    assert call(dim=8 * 65) != 0 and b"exceeds 64" in _err()
    assert call(codes=16392) != 0 and b"16-byte aligned" in _err()
    for nlist in (0, -1, 1 << 24):
        assert call(nlist=nlist) != 0 and b"nlist=" in _err() and b"outside [1, 2^24)" in _err()
    for nprobe in (0, -1, 17):
        assert call(nprobe=nprobe) != 0 and b"nprobe=" in _err() and b"outside [1, min(nlist=16, 1024)]" in _err()
    assert call(nlist=4096, nprobe=1025) != 0 and b"outside [1, min(nlist=4096, 1024)]" in _err()
    assert call(cap=0) != 0 and b"cap=0" in _err()
    for k in (0, -1, 501, 1025):
        assert call(k=k) != 0 and b"outside [1, 500]" in _err()
    assert call(cap=5000, k=1025) != 0 and b"outside [1, 1024]" in _err()
    assert call(Q=1 << 29, nprobe=4) != 0 and b"too large" in _err()                  # Q * nprobe >= 2^31
    assert call(Q=1 << 20, nprobe=1, cap=(1 << 20) + 1) != 0 and b"too large" in _err()   # Q * cap > 2^40
    filt.label_mode = 7
    assert call(f=ctypes.byref(filt)) != 0 and b"label_mode" in _err()
    filt.label_mode = _lib.LABEL_SAME
    assert call(f=ctypes.byref(filt)) != 0 and b"needs query_labels" in _err()
    assert call(ws_bytes=1024) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()
    assert call(cap=5000, k=1024, ws_bytes=1024) != 0 and b"workspace" in _err()
    assert call(Q=0, ws=None, ws_bytes=0) == 0                                        # nothing to do


def _trained(dim=64, m=8, rows=500, device="cpu"):
    g = pq.PQGallery(dim, device, m)
    g._codebooks = torch.zeros(m, 256, dim // m, device=device)                       # as if trained
    g.rows = rows                                                                     # as if rows had been added
    return g


def test_build_checks_its_arguments():
    g = _trained()
    with pytest.raises(MI355Error, match="built over a PQGallery"):
        ivfpq.IVFPQIndex.build(Gallery(64, "cpu"), torch.zeros(500, 64), 4)
    with pytest.raises(MI355Error, match="no codebooks"):
        ivfpq.IVFPQIndex.build(pq.PQGallery(64, "cpu", 8), torch.zeros(500, 64), 4)
    with pytest.raises(MI355Error, match="at least one row"):
        ivfpq.IVFPQIndex.build(_trained(rows=0), torch.zeros(0, 64), 4)
    with pytest.raises(MI355Error, match="Gallery or a tensor"):
        ivfpq.IVFPQIndex.build(g, [[0.0] * 64] * 500, 4)
    with pytest.raises(MI355Error, match="must be fp32"):
        ivfpq.IVFPQIndex.build(g, torch.zeros(500, 64, dtype=torch.float16), 4)
    with pytest.raises(MI355Error, match="rows are on meta"):
        ivfpq.IVFPQIndex.build(g, torch.zeros(500, 64, device="meta"), 4)
    with pytest.raises(MI355Error, match="rows are on meta"):
        g.ivf(Gallery(64, "meta"), 4)                                                 # the convenience goes the same way
    with pytest.raises(MI355Error, match="rows have dim 32"):
        ivfpq.IVFPQIndex.build(g, torch.zeros(500, 32), 4)
    with pytest.raises(MI355Error, match=r"\(N, 64\)"):
        ivfpq.IVFPQIndex.build(g, torch.zeros(500), 4)
    with pytest.raises(MI355Error, match="rows holds 499 rows"):
        ivfpq.IVFPQIndex.build(g, torch.zeros(499, 64), 4)
    short = Gallery(64, "cpu")
    short.rows = 499
    with pytest.raises(MI355Error, match="rows holds 499 rows"):
        ivfpq.IVFPQIndex.build(g, short, 4)
    with pytest.raises(MI355Error, match="built over a PQGallery"):
        ivfpq.IVFPQIndex(Gallery(64, "cpu"), torch.zeros(4, 64), torch.zeros(500, dtype=torch.int64))
    with pytest.raises(MI355Error, match=r"centroids must be \(nlist, 64\)"):
        ivfpq.IVFPQIndex(g, torch.zeros(4, 32), torch.zeros(500, dtype=torch.int64))
    with pytest.raises(MI355Error, match="centroids must be a tensor"):
        ivfpq.IVFPQIndex(g, None, torch.zeros(500, dtype=torch.int64))


def _index(rows=500, nlist=16):
    """An index as if built, without the GPU: 16 lists of rows // 16 rows (the first takes the remainder)."""
    ix = object.__new__(ivfpq.IVFPQIndex)
    ix.pq = _trained(rows=rows)
    ix.nlist, ix.rows = nlist, rows
    counts = np.full(nlist, rows // nlist)
    counts[0] += rows - counts.sum()
    ix._longest = np.concatenate([[0], np.cumsum(np.sort(counts)[::-1])])
    ix.centroids = torch.zeros(nlist, 64)
    return ix


def test_search_checks_its_arguments():
    ix = _index()
    q = torch.zeros(2, 64)
    for kw in ({}, {"nprobe": 2, "probes": torch.zeros(2, 2, dtype=torch.int64)}):
        with pytest.raises(MI355Error, match="exactly one of nprobe and probes"):
            ix.search(q, 3, **kw)
    for nprobe in (0, 17, -1, 1.5, True):
        with pytest.raises(MI355Error, match=r"outside \[1, 16\]"):
            ix.search(q, 3, nprobe)
        with pytest.raises(MI355Error, match=r"outside \[1, 16\]"):
            ix.probe(q, nprobe)
    with pytest.raises(MI355Error, match=r"outside \[1, 16\]"):
        ix.search(q, 3, probes=torch.zeros(2, 17, dtype=torch.int64))
    with pytest.raises(MI355Error, match=r"probes must be a \(Q, nprobe\) tensor"):
        ix.search(q, 3, probes=torch.zeros(2, dtype=torch.int64))
    big = _index(rows=5000, nlist=2000)
    with pytest.raises(MI355Error, match=r"outside \[1, 1024\]"):
        big.search(q, 3, 1025)
    for k in (0, 501, 1.5, True):
        with pytest.raises(MI355Error, match="k out of range"):
            ix.search(q, k, 2)
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        ix.search(q, 3, 2, refine=torch.zeros(500, 64))
    with pytest.raises(MI355Error, match="refine is on"):
        ix.search(q, 3, 2, refine=Gallery(64, "meta"))
    other = Gallery(64, "cpu")
    other.rows = 499
    with pytest.raises(MI355Error, match="refine holds 499 rows"):
        ix.search(q, 3, 2, refine=other)
    other.rows = 500
    with pytest.raises(MI355Error, match="shortlist=2 outside"):
        ix.search(q, 3, 2, refine=other, shortlist=2)
    with pytest.raises(MI355Error, match="shortlist=501 outside"):
        ix.search(q, 3, 2, refine=other, shortlist=501)
    with pytest.raises(MI355Error, match="give refine too"):
        ix.search(q, 3, 2, shortlist=100)
    with pytest.raises(MI355Error, match="same 500 rows"):
        ix.recall(q, 3, 2, exact=Gallery(64, "cpu"))


def test_a_stale_index_refuses_to_search():
    ix = _index()
    assert not ix.stale
    ix.pq.rows = 501                                                                  # as if pq.add had run behind its back
    assert ix.stale
    with pytest.raises(MI355Error, match="stale: it lists 500 rows but the PQGallery holds 501"):
        ix.search(torch.zeros(2, 64), 3, 2)
    with pytest.raises(MI355Error, match="stale"):
        ix.add(torch.zeros(1, 64))


def test_export_is_lazy_and_not_in_all():
    assert "IVFPQIndex" not in M.__all__
    assert M.IVFPQIndex is ivfpq.IVFPQIndex
    assert pq.PQGallery.ivf is not None
