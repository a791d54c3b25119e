"""Residual IVF-PQ, the parts that need no GPU: the C-ABI symbols, every argument check of the two new entries (rejected before any
HIP call, with a message), the sizer, the Python-side checks and the export."""
import ctypes

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, MI355Error, _lib, ivfpq, ivfrpq, pq

NEW = ["mi355_ivfpq_residuals", "mi355_ivfpq_residual_search_workspace_bytes", "mi355_ivfpq_residual_search"]
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
    assert ivfrpq.ENCODE_BLOCK == 16384


def test_workspace_sizes():
    s = _lib.lib().mi355_ivfpq_residual_search_workspace_bytes          # (Q, nprobe, nlist, dim, M, cap, k)
    plain = _lib.lib().mi355_ivfpq_search_workspace_bytes
    assert s(0, 8, 256, 1536, 96, 5000, 3) == 0                                       # Q = 0
    for k in (3, 150):
        for Q, nprobe, cap in ((1, 8, 5000), (16, 8, 5000), (256, 32, 100000), (1000, 1, 700), (300, 1024, 10 ** 6)):
            # the plain search's bytes and the coarse terms of one query block, rounded up to 256
            qb = min(Q, 256, max(1, (1 << 29) // (12 * cap))) if k > 8 else min(Q, 256)
            assert s(Q, nprobe, 1024, 1536, 96, cap, k) == plain(Q, nprobe, 1024, 1536, 96, cap, k) + -(-qb * nprobe * 4 // 256) * 256
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
             cap=500, k=3, f=None, cen=36864, out=32768, out_idx=49152, ws=65536, ws_bytes=BIG):
        return L.mi355_ivfpq_residual_search(q, Q, dim, 1e-6, cb, M, codes, G, offsets, order, nlist, probes, nprobe, cap, k, 0, f,
                                             cen, out, out_idx, ws, ws_bytes, None)

    for name in ("q", "cb", "codes", "offsets", "order", "probes", "cen", "out", "out_idx"):
        assert call(**{name: None}) != 0 and b"ivfpq_residual_search: null" in _err(), name
    assert call(Q=-1) != 0 and b"bad shape" in _err()
    assert call(G=0) != 0 and b"bad shape" in _err()
    assert call(M=6) != 0 and b"multiple of 4" in _err()                              # the PQ shape rules
    assert call(M=132, dim=132 * 4) != 0 and b"multiple of 4 in [4, 128]" in _err()
    assert call(dim=66) != 0 and b"multiple of M" in _err()
    assert call(dim=0) != 0 and _err()
    assert call(dim=8 * 65) != 0 and b"exceeds 64" in _err()
    assert call(codes=16392) != 0 and b"16-byte aligned" in _err()                    # an unaligned list_codes
    for nlist in (0, -1, 1 << 24):
        assert call(nlist=nlist) != 0 and b"nlist=" in _err() and b"outside [1, 2^24)" in _err()
    for nprobe in (0, -1, 17):                                                        # nprobe > nlist
        assert call(nprobe=nprobe) != 0 and b"nprobe=" in _err() and b"outside [1, min(nlist=16, 1024)]" in _err()
    assert call(nlist=4096, nprobe=1025) != 0 and b"outside [1, min(nlist=4096, 1024)]" in _err()     # nprobe > 1024
    assert call(cap=0) != 0 and b"cap=0" in _err()
    for k in (0, -1, 501, 1025):                                                      # k > cap
        assert call(k=k) != 0 and b"outside [1, 500]" in _err()
    assert call(cap=5000, k=1025) != 0 and b"outside [1, 1024]" in _err()
    assert call(Q=1 << 29, nprobe=4) != 0 and b"too large" in _err()
    filt.label_mode = 7
    assert call(f=ctypes.byref(filt)) != 0 and b"label_mode" in _err()
    assert call(ws_bytes=1024) != 0 and b"workspace" in _err()                        # a workspace that is too small
    assert call(ws=None) != 0 and b"workspace" in _err()
    need = L.mi355_ivfpq_residual_search_workspace_bytes(8, 4, 16, 64, 8, 500, 3)
    assert call(ws_bytes=need - 1) != 0 and b"workspace" in _err()
    assert call(ws_bytes=L.mi355_ivfpq_search_workspace_bytes(8, 4, 16, 64, 8, 500, 3)) != 0 and b"workspace" in _err()
    assert call(Q=0, ws=None, ws_bytes=0) == 0                                        # nothing to do


def test_residuals_argument_errors():
    L = _lib.lib()

    def call(rows=4096, R=100, dim=64, normalized=0, a=8192, cen=12288, nlist=16, out=16384, ws=20480, ws_bytes=512):
        return L.mi355_ivfpq_residuals(rows, R, dim, normalized, 1e-6, a, cen, nlist, out, ws, ws_bytes, None)

    for name in ("rows", "a", "cen", "out"):
        assert call(**{name: None}) != 0 and b"ivfpq_residuals: null" in _err(), name
    assert call(R=-1) != 0 and b"bad shape" in _err()
    assert call(R=(1 << 31) + 1) != 0 and b"bad shape" in _err()
    for dim in (0, -4, 8193):
        assert call(dim=dim) != 0 and b"bad shape" in _err()
    for nlist in (0, -1, 1 << 24):
        assert call(nlist=nlist) != 0 and b"outside [1, 2^24)" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()
    assert call(ws_bytes=511) != 0 and b"workspace 511 < 512" in _err()
    assert call(R=0, ws=None, ws_bytes=0) == 0                                        # nothing to do


def _index(rows=500, nlist=16, device="cpu"):
    """An index as if built, without the GPU: 16 lists of rows // 16 rows (the first takes the remainder)."""
    ix = object.__new__(ivfrpq.ResidualIVFPQIndex)
    ix.pq = object.__new__(ivfrpq._ResidualCodes)
    pq.PQGallery.__init__(ix.pq, 64, device, 8)
    ix.pq._codebooks = torch.zeros(8, 256, 8, device=device)                          # as if trained
    ix.pq.rows = rows                                                                 # as if rows had been added
    ix.nlist, ix.rows = nlist, rows
    counts = np.full(nlist, rows // nlist)
    counts[0] += rows - counts.sum()
    ix._longest = np.concatenate([[0], np.cumsum(np.sort(counts)[::-1])])
    ix.centroids = torch.zeros(nlist, 64, device=device)
    return ix


def test_search_checks_its_arguments():
    ix = _index()
    q = torch.zeros(2, 64)
    for kw in ({}, {"nprobe": 2, "probes": torch.zeros(2, 2, dtype=torch.int64)}):
        with pytest.raises(MI355Error, match="exactly one of nprobe and probes"):
            ix.search(q, 3, **kw)
    with pytest.raises(MI355Error, match="exactly one of nprobe and probes"):
        ix.coarse(q, None)
    for nprobe in (0, 17, -1, 1.5, True):
        with pytest.raises(MI355Error, match=r"outside \[1, 16\]"):
            ix.search(q, 3, nprobe)
    with pytest.raises(MI355Error, match=r"outside \[1, 16\]"):
        ix.coarse(q, torch.zeros(2, 17, dtype=torch.int64))
    with pytest.raises(MI355Error, match=r"queries must be \(Q, 64\)"):
        ix.search(torch.zeros(2, 32), 3, 2)                                           # a wrong dim
    with pytest.raises(MI355Error, match="queries are on meta but the index lives on cpu"):
        ix.search(torch.zeros(2, 64, device="meta"), 3, 2)                            # a wrong device
    for k in (0, 501, 1.5, True):
        with pytest.raises(MI355Error, match="k out of range"):
            ix.search(q, k, 2)
    with pytest.raises(MI355Error, match="give refine too"):
        ix.search(q, 3, 2, shortlist=100)                                             # shortlist without refine
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        ix.search(q, 3, 2, refine=torch.zeros(500, 64))
    other = Gallery(64, "cpu")
    other.rows = 499
    with pytest.raises(MI355Error, match="refine holds 499 rows"):
        ix.search(q, 3, 2, refine=other)
    for exact in (None, Gallery(64, "cpu")):
        with pytest.raises(MI355Error, match="same 500 rows"):
            ix.recall(q, 3, 2, exact)


def test_add_checks_its_arguments():
    ix = _index()
    with pytest.raises(MI355Error, match=r"embeddings must be a \(n, 64\) tensor"):
        ix.add(torch.zeros(5, 32))                                                    # a wrong dim
    with pytest.raises(MI355Error, match=r"embeddings must be a \(n, 64\) tensor"):
        ix.add([[0.0] * 64])
    for a in (torch.zeros(4, dtype=torch.int64), torch.zeros(6, dtype=torch.int64), torch.zeros(5, 1, dtype=torch.int64), [0] * 5):
        with pytest.raises(MI355Error, match=r"assignments must have shape \(5,\)"):
            ix.add(torch.zeros(5, 64), assignments=a)                                 # assignments of the wrong length
    with pytest.raises(MI355Error, match="embeddings are on meta but the index lives on cpu"):
        ix.add(torch.zeros(5, 64, device="meta"))                                     # a wrong device
    ix.pq.rows = 501                                                                  # rows behind the index's back
    with pytest.raises(MI355Error, match="stale"):
        ix.add(torch.zeros(5, 64))
    with pytest.raises(MI355Error, match="stale"):
        ix.search(torch.zeros(2, 64), 3, 2)


def test_build_checks_its_arguments():
    B = ivfrpq.ResidualIVFPQIndex.build
    with pytest.raises(MI355Error, match="rows must be fp32"):
        B(torch.zeros(500, 64, dtype=torch.float16), 8, 4)                            # fp16 rows
    with pytest.raises(MI355Error, match="fp16 Gallery"):
        B(Gallery(64, "cpu", dtype=torch.float16), 8, 4)
    with pytest.raises(MI355Error, match="fp16 Gallery"):
        ivfrpq.ResidualIVFPQIndex.from_gallery(Gallery(64, "cpu", dtype=torch.float16), 8, 4)
    with pytest.raises(MI355Error, match="from_gallery needs a Gallery"):
        ivfrpq.ResidualIVFPQIndex.from_gallery(torch.zeros(500, 64), 8, 4)
    with pytest.raises(MI355Error, match="Gallery or a tensor"):
        B([[0.0] * 64] * 500, 8, 4)
    with pytest.raises(MI355Error, match=r"rows must be \(N, D\)"):
        B(torch.zeros(500), 8, 4)
    with pytest.raises(MI355Error, match="multiple of 4"):
        B(torch.zeros(500, 64), 6, 4)
    with pytest.raises(MI355Error, match="positive multiple of M"):
        B(torch.zeros(500, 66), 8, 4)                                                 # a wrong dim
    with pytest.raises(MI355Error, match="pq_iters"):
        B(torch.zeros(500, 64), 8, 4, pq_iters=-1)
    for train_rows in (255, 501, 300.0, True):
        with pytest.raises(MI355Error, match=r"train_rows in \[256, N\]"):
            B(torch.zeros(500, 64), 8, 4, train_rows=train_rows)
    with pytest.raises(MI355Error, match=r"train_rows in \[256, N\]"):
        B(torch.zeros(200, 64), 8, 4)                                                 # too few rows to seed 256 centroids
    with pytest.raises(MI355Error, match="must live on the GPU"):
        B(torch.zeros(500, 64), 8, 4)                                                 # a wrong device: found before any launch


def test_constructor_checks_its_arguments():
    C = ivfrpq.ResidualIVFPQIndex
    with pytest.raises(MI355Error, match=r"centroids must be a \(nlist, D\) tensor"):
        C(None, torch.zeros(8, 256, 8))
    with pytest.raises(MI355Error, match=r"centroids must be a \(nlist, D\) tensor"):
        C(torch.zeros(0, 64), torch.zeros(8, 256, 8))
    with pytest.raises(MI355Error, match=r"codebooks must be a \(M, 256, D / M\) tensor"):
        C(torch.zeros(4, 64), torch.zeros(8, 256))
    with pytest.raises(MI355Error, match="must live on the GPU"):
        C(torch.zeros(4, 64), torch.zeros(8, 256, 8))


def test_export_is_lazy_and_not_in_all():
    assert "ResidualIVFPQIndex" not in M.__all__
    assert M.ResidualIVFPQIndex is ivfrpq.ResidualIVFPQIndex
    assert issubclass(ivfrpq.ResidualIVFPQIndex, ivfpq.IVFPQIndex)
    for name in ("build", "add", "search", "probe", "coarse", "recall", "reconstruct", "codes", "list_codes", "codebooks", "labels",
                 "nbytes"):
        assert hasattr(ivfrpq.ResidualIVFPQIndex, name), name
