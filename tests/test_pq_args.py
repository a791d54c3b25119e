"""Product-quantised gallery, the parts that need no GPU: the C-ABI symbols, every argument check of the new entries (rejected
before any HIP call, with a message), the workspace sizes, the Python-side checks and the export."""
import ctypes

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, MI355Error, _lib, pq

NEW = ["mi355_pq_encode_workspace_bytes", "mi355_pq_encode", "mi355_pq_update_workspace_bytes", "mi355_pq_update",
       "mi355_pq_search_workspace_bytes", "mi355_pq_scores", "mi355_pq_search", "mi355_rescore_candidates_workspace_bytes",
       "mi355_rescore_candidates"]
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


def test_workspace_sizes():
    L = _lib.lib()
    s = L.mi355_pq_search_workspace_bytes
    assert s(0, 1000, 64, 8, 3) == 0 and s(0, 1000, 64, 8, 0) == 0                     # Q = 0
    for k in (0, 3, 150):                                                             # monotone in Q, G and M
        assert 0 < s(1, 1000, 1536, 48, k) <= s(16, 1000, 1536, 48, k) <= s(256, 1000, 1536, 48, k) <= s(1000, 1000, 1536, 48, k)
        assert s(16, 1000, 1536, 48, k) <= s(16, 100000, 1536, 48, k) <= s(16, 1000000, 1536, 48, k)
        assert s(16, 1000, 1536, 48, k) <= s(16, 1000, 1536, 96, k)
    assert s(256, 100000, 1536, 96, 3) < 64 << 20                                     # k <= 8: tables and candidates, no slab
    assert s(256, 100000, 1536, 96, 150) > 256 * 100000 * 4                           # the score slab
    assert s(256, 100000, 1536, 96, 0) >= 256 * 96 * 1024                             # the tables of a query block
    for bad in ((4, 10, 64, 6, 1), (4, 10, 64, 132, 1), (4, 10, 66, 8, 1), (4, 10, 1024, 8, 1), (4, 10, 64, 8, 1025),
                (4, 10, 64, 8, -1), (4, -1, 64, 8, 1), (4, 10, 0, 8, 1)):
        assert s(*bad) == 0, bad
    e, u, r = L.mi355_pq_encode_workspace_bytes, L.mi355_pq_update_workspace_bytes, L.mi355_rescore_candidates_workspace_bytes
    assert e(0, 64, 0) == 0 and u(0, 64, 0) == 0 and r(0, 64) == 0
    assert e(10, 64, 1) == 0 and u(10, 64, 1) == 0                                    # normalised rows are read where they lie
    assert 0 < e(10, 64, 0) <= e(1000, 64, 0) <= e(10 ** 6, 64, 0) < 10 ** 6 * 64 * 4  # rows are normalised a block at a time
    assert 10 * 64 * 4 <= u(10, 64, 0) <= u(1000, 64, 0)
    assert 10 * 64 * 4 <= r(10, 64) <= r(1000, 64)


def _shape_errors(call):
    assert call(M=6) != 0 and b"multiple of 4" in _err()
    assert call(M=0) != 0 and b"multiple of 4" in _err()
    assert call(M=132, dim=132 * 4) != 0 and b"multiple of 4 in [4, 128]" in _err()
    assert call(dim=66) != 0 and b"multiple of M" in _err()
    assert call(dim=0) != 0 and _err()
    assert call(dim=8 * 65) != 0 and b"exceeds 64" in _err()


def test_encode_argument_errors():
    L = _lib.lib()

    def call(rows=4096, R=4, dim=64, M=8, norm=0, cb=8192, codes=16384, codes_bytes=BIG, ws=65536, ws_bytes=BIG):
        return L.mi355_pq_encode(rows, R, dim, M, norm, 1e-6, cb, codes, codes_bytes, ws, ws_bytes, None)

    for name in ("rows", "cb", "codes"):
        assert call(**{name: None}) != 0 and b"null" in _err()
    assert call(R=-1) != 0 and b"bad shape" in _err()
    _shape_errors(call)
    assert call(codes_bytes=4 * 8 - 1) != 0 and b"output buffer" in _err()
    assert call(ws_bytes=16) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()
    assert call(R=0, ws=None, ws_bytes=0) == 0                                        # nothing to do
    assert call(R=0, norm=1, ws=None, ws_bytes=0) == 0


def test_update_argument_errors():
    L = _lib.lib()

    def call(rows=4096, R=4, dim=64, M=8, norm=0, codes=16384, cb=8192, out=8192, counts=32768, ws=65536, ws_bytes=BIG):
        return L.mi355_pq_update(rows, R, dim, M, norm, 1e-6, codes, cb, out, counts, ws, ws_bytes, None)

    for name in ("rows", "codes", "cb", "out", "counts"):
        assert call(**{name: None}) != 0 and b"null" in _err()
    assert call(R=-1) != 0 and b"bad shape" in _err()
    _shape_errors(call)
    assert call(codes=16388) != 0 and b"16-byte aligned" in _err()
    assert call(ws_bytes=16) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()
    assert call(R=0, ws=None, ws_bytes=0) == 0


def test_scores_and_search_argument_errors():
    L = _lib.lib()
    filt = _lib.RankFilter()

    def scores(q=4096, Q=8, dim=64, cb=8192, M=8, codes=16384, G=100, out=32768, ws=65536, ws_bytes=BIG):
        return L.mi355_pq_scores(q, Q, dim, 1e-6, cb, M, codes, G, out, ws, ws_bytes, None)

    def search(q=4096, Q=8, dim=64, cb=8192, M=8, codes=16384, G=100, k=3, f=None, out=32768, out_idx=49152, ws=65536, ws_bytes=BIG):
        return L.mi355_pq_search(q, Q, dim, 1e-6, cb, M, codes, G, k, 0, f, out, out_idx, ws, ws_bytes, None)

    for call in (scores, search):
        for name in ("q", "cb", "codes", "out"):
            assert call(**{name: None}) != 0 and b"null" in _err()
        assert call(Q=-1) != 0 and b"bad shape" in _err()
        assert call(G=-1) != 0 and b"bad shape" in _err()
        _shape_errors(call)
        assert call(codes=16392) != 0 and b"16-byte aligned" in _err()
        assert call(ws_bytes=1024) != 0 and b"workspace" in _err()
        assert call(ws=None) != 0 and b"workspace" in _err()
        assert call(Q=0, ws=None, ws_bytes=0) == 0                                    # nothing to do
        assert call(G=0, ws=None, ws_bytes=0) == 0
    assert search(out_idx=None) != 0 and b"null" in _err()
    for k in (0, -1, 101, 1025):
        assert search(k=k) != 0 and b"outside [1, 100]" in _err()
    assert search(G=5000, k=1025) != 0 and b"outside [1, 1024]" in _err()
    assert search(G=5000, k=1024, ws_bytes=1024) != 0 and b"workspace" in _err()
    filt.label_mode = 7
    assert search(f=ctypes.byref(filt)) != 0 and b"label_mode" in _err()
    filt.label_mode = _lib.LABEL_SAME
    assert search(f=ctypes.byref(filt)) != 0 and b"needs query_labels" in _err()


def test_rescore_argument_errors():
    L = _lib.lib()

    def call(q=4096, Q=8, dim=64, rows=8192, dtype=0, ld=64, G=100, cand=16384, R=10, out=32768, ws=65536, ws_bytes=BIG):
        return L.mi355_rescore_candidates(q, Q, dim, 1e-6, rows, dtype, ld, G, cand, R, 0, out, ws, ws_bytes, None)

    for name in ("q", "rows", "cand", "out"):
        assert call(**{name: None}) != 0 and b"null" in _err()
    assert call(dtype=2) != 0 and b"unknown rows dtype" in _err()
    assert call(Q=-1) != 0 and b"bad shape" in _err()
    assert call(R=-1) != 0 and b"bad shape" in _err()
    assert call(dim=0) != 0 and b"bad shape" in _err()
    assert call(ld=63) != 0 and b"ld=63 < dim" in _err()
    assert call(dtype=1, rows=8200) != 0 and b"16-byte aligned" in _err()
    assert call(dtype=1, ld=68) != 0 and b"multiple of 8" in _err()
    assert call(dim=20000, ld=20000) != 0 and b"too large" in _err()
    assert call(ws_bytes=16) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()
    assert call(Q=0, ws=None, ws_bytes=0) == 0
    assert call(R=0) == 0


def test_pqgallery_checks_its_shape():
    for dim, m in ((64, 6), (64, 0), (66, 8), (8 * 65, 8), (132 * 4, 132), (0, 4)):
        with pytest.raises(MI355Error):
            pq.PQGallery(dim, "cpu", m)
    g = pq.PQGallery(1536, "cpu", 96, capacity=3)
    assert (g.dsub, len(g), g.codebooks, g.labels) == (16, 0, None, None) and g.codes.shape == (0, 96) and g.nbytes == 3 * 96


def test_pqgallery_errors():
    g = pq.PQGallery(64, "cpu", 8)
    with pytest.raises(MI355Error, match="no codebooks"):
        g.add(torch.zeros(3, 64))
    with pytest.raises(MI355Error, match="no codebooks"):
        g.search(torch.zeros(3, 64), 1)
    with pytest.raises(MI355Error, match="no codebooks"):
        g.scores(torch.zeros(3, 64))
    with pytest.raises(MI355Error, match="cannot seed 256"):
        g.train(torch.zeros(255, 64))
    with pytest.raises(MI355Error, match="fp32"):
        g.train(torch.zeros(300, 64, dtype=torch.float16))
    with pytest.raises(MI355Error, match="fp16 Gallery"):
        g.train(Gallery(64, "cpu", dtype=torch.float16))
    with pytest.raises(MI355Error, match=r"\(N, 64\)"):
        g.train(torch.zeros(300, 32))
    g._codebooks = torch.zeros(8, 256, 8)                                             # as if trained
    g.rows = 500                                                                      # as if rows had been added
    with pytest.raises(MI355Error, match="already resident"):
        g.train(torch.zeros(300, 64))
    q = torch.zeros(2, 64)
    for k in (0, 501, 1.5, True):
        with pytest.raises(MI355Error, match="k out of range"):
            g.search(q, k)
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        g.search(q, 3, refine=torch.zeros(500, 64))
    with pytest.raises(MI355Error, match="refine is on"):
        g.search(q, 3, refine=Gallery(64, "meta"))
    other = Gallery(64, "cpu")
    other.rows = 499
    with pytest.raises(MI355Error, match="refine holds 499 rows"):
        g.search(q, 3, refine=other)
    other.rows = 500
    with pytest.raises(MI355Error, match="shortlist=2 outside"):
        g.search(q, 3, refine=other, shortlist=2)
    with pytest.raises(MI355Error, match="shortlist=501 outside"):
        g.search(q, 3, refine=other, shortlist=501)
    with pytest.raises(MI355Error, match="give refine too"):
        g.search(q, 3, shortlist=100)
    with pytest.raises(MI355Error, match="same 500 rows"):
        g.recall(q, 3, Gallery(64, "cpu"))


def test_export_is_lazy_and_not_in_all():
    assert "PQGallery" not in M.__all__
    assert M.PQGallery is pq.PQGallery
