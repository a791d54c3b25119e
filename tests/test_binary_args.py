"""Binary gallery, the parts that need no GPU: the C-ABI symbols, every argument check of the new entries (rejected before any
HIP call, with a message), the sizers, the Python-side checks and the export."""
import ctypes

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, MI355Error, _lib, binary

NEW = ["mi355_binary_bytes", "mi355_binary_encode", "mi355_binary_search_workspace_bytes", "mi355_binary_distances",
       "mi355_binary_search"]
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


def test_sizers():
    L = _lib.lib()
    b = L.mi355_binary_bytes
    # ceil(dim / 32) words rounded up to 4: 16-byte rows
    for dim, ld in ((1, 4), (32, 4), (96, 4), (128, 4), (129, 8), (130, 8), (1000, 32), (1536, 48), (2560, 80), (65536, 2048)):
        assert b(1, dim) == ld * 4 and b(1000, dim) == 1000 * ld * 4, dim
        assert binary.row_words(dim) == ld and binary.words(dim) == (dim + 31) // 32
    for bad in ((0, 64), (-1, 64), (10, 0), (10, -3), (10, 65537), (BIG + 1, 64)):
        assert b(*bad) == 0, bad
    s = L.mi355_binary_search_workspace_bytes
    assert s(0, 1000, 64, 3) == 0 and s(0, 1000, 64, 0) == 0                          # Q = 0
    for k in (0, 3, 150):                                                             # monotone in Q, G and dim
        assert 0 < s(1, 1000, 1536, k) <= s(16, 1000, 1536, k) <= s(256, 1000, 1536, k) <= s(1000, 1000, 1536, k)
        assert s(16, 1000, 1536, k) <= s(16, 100000, 1536, k) <= s(16, 1000000, 1536, k)
        assert s(16, 1000, 64, k) <= s(16, 1000, 1536, k) <= s(16, 1000, 2560, k)
    assert s(256, 1000000, 1536, 3) < 64 << 20                                        # k <= 8: candidates, no slab
    assert s(256, 1000000, 1536, 150) < 256 << 20                                     # k > 8: 8 per chunk + 18 chunks, no slab
    assert s(256, 1000000, 1536, 3) < s(256, 1000000, 1536, 150) < s(256, 1000000, 1536, 1024)
    assert 256 * 192 <= s(256, 100000, 1536, 0) < 1 << 20                             # distances: the queries' codes only
    for bad in ((4, 10, 0, 1), (4, 10, 65537, 1), (4, 10, 64, 1025), (4, 10, 64, -1), (4, -1, 64, 1), (-1, 10, 64, 1),
                (4, 1 << 31, 64, 1), (1 << 31, 10, 64, 1)):
        assert s(*bad) == 0, bad


def test_encode_argument_errors():
    L = _lib.lib()

    def call(rows=4096, R=4, dim=64, norm=0, center=8192, codes=16384, codes_bytes=BIG):
        return L.mi355_binary_encode(rows, R, dim, norm, 1e-6, center, codes, codes_bytes, None)

    for name in ("rows", "codes"):
        assert call(**{name: None}) != 0 and b"null" in _err()
    assert call(R=-1) != 0 and b"bad shape" in _err()
    assert call(dim=0) != 0 and b"bad shape" in _err()
    assert call(dim=65537) != 0 and b"exceeds 65536" in _err()
    assert call(R=BIG + 1) != 0 and b"too large" in _err()
    assert call(codes=16388) != 0 and b"16-byte aligned" in _err()
    assert call(codes_bytes=4 * 16 - 1) != 0 and b"output buffer" in _err()
    assert call(dim=130, codes_bytes=4 * 32 - 1) != 0 and b"output buffer" in _err()  # 5 words are stored as 8
    assert call(R=0) == 0                                                             # nothing to do
    assert call(R=0, center=None, norm=1, codes_bytes=0) == 0


def test_distances_and_search_argument_errors():
    L = _lib.lib()
    filt = _lib.RankFilter()

    def distances(q=4096, Q=8, dim=64, center=8192, codes=16384, G=100, out=32768, ws=65536, ws_bytes=BIG):
        return L.mi355_binary_distances(q, Q, dim, 1e-6, center, codes, G, out, ws, ws_bytes, None)

    def search(q=4096, Q=8, dim=64, center=8192, codes=16384, G=100, k=3, f=None, out=32768, out_idx=49152, ws=65536, ws_bytes=BIG):
        return L.mi355_binary_search(q, Q, dim, 1e-6, center, codes, G, k, 0, f, out, out_idx, ws, ws_bytes, None)

    for call in (distances, search):
        for name in ("q", "codes", "out"):
            assert call(**{name: None}) != 0 and b"null" in _err()
        assert call(Q=-1) != 0 and b"bad shape" in _err()
        assert call(G=-1) != 0 and b"bad shape" in _err()
        assert call(dim=0) != 0 and b"bad shape" in _err()
        assert call(dim=65537) != 0 and b"exceeds 65536" in _err()
        assert call(G=1 << 31) != 0 and b"too large" in _err()
        assert call(Q=1 << 31) != 0 and b"too large" in _err()
        assert call(codes=16392) != 0 and b"16-byte aligned" in _err()
        assert call(ws_bytes=64) != 0 and b"workspace" in _err()
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


def test_binarygallery_checks_its_shape():
    for dim in (0, -1, 65537, 1.5, True, "64"):
        with pytest.raises(MI355Error, match="dim in"):
            binary.BinaryGallery(dim, "cpu")
    g = binary.BinaryGallery(1536, "cpu", capacity=3)
    assert (g.W, len(g), g.center, g.labels) == (48, 0, None, None)
    assert g.codes.shape == (0, 48) and g.codes.dtype == torch.int32 and g.nbytes == 3 * 192
    g = binary.BinaryGallery(130, "cpu", capacity=2)
    assert g.codes.shape == (0, 5) and g._codes.shape == (2, 8) and g.nbytes == 2 * 32
    g._center = torch.zeros(130)                                                      # as if trained
    assert g.nbytes == 2 * 32 + 130 * 4
    with pytest.raises(MI355Error, match="center must live on the GPU"):
        binary.BinaryGallery(130, "cpu", center=torch.zeros(130))


def test_binarygallery_errors():
    with pytest.raises(MI355Error, match=r"center must be \(64,\)"):
        binary.BinaryGallery(64, "cpu", center=torch.zeros(63))
    with pytest.raises(MI355Error, match=r"center must be \(64,\)"):
        binary.BinaryGallery(64, "cpu", center=torch.zeros(1, 64))
    with pytest.raises(MI355Error, match=r"center must be \(64,\) on cpu"):
        binary.BinaryGallery(64, "cpu", center=torch.zeros(64, device="meta"))
    with pytest.raises(MI355Error, match="center must be"):
        binary.BinaryGallery(64, "cpu", center=[0.0] * 64)
    g = binary.BinaryGallery(64, "cpu")
    with pytest.raises(MI355Error, match="embeddings must live on the GPU"):         # (shapes: tests/test_binary_gpu.py)
        g.add(torch.zeros(3, 64))
    with pytest.raises(MI355Error, match="fp32"):
        g.train(torch.zeros(300, 64, dtype=torch.float16))
    with pytest.raises(MI355Error, match="fp16 Gallery"):
        g.train(Gallery(64, "cpu", dtype=torch.float16))
    with pytest.raises(MI355Error, match=r"\(N, 64\)"):
        g.train(torch.zeros(300, 32))
    with pytest.raises(MI355Error, match=r"\(N, 64\)"):
        g.train(torch.zeros(300, 64, device="meta"))
    with pytest.raises(MI355Error, match="no rows"):
        g.train(torch.zeros(0, 64))
    with pytest.raises(MI355Error, match="tensor or a Gallery"):
        g.train([[0.0] * 64])
    with pytest.raises(MI355Error, match=r"the Gallery is \(32,\)"):
        g.train(Gallery(32, "cpu"))
    with pytest.raises(MI355Error, match="needs a Gallery"):
        binary.BinaryGallery.from_gallery(torch.zeros(3, 64))
    g.rows = 500                                                                      # as if rows had been added
    with pytest.raises(MI355Error, match="already resident"):
        g.train(torch.zeros(300, 64))
    q = torch.zeros(2, 64)
    for k in (0, 501, 1.5, True):
        with pytest.raises(MI355Error, match="k out of range"):
            g.search(q, k)
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        g.search(q, 3, refine=torch.zeros(500, 64))
    with pytest.raises(MI355Error, match="refine is on meta but the BinaryGallery"):
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
    for call in (lambda x: g.search(x, 3), g.distances):
        with pytest.raises(MI355Error, match="queries must live on the GPU"):
            call(q)


def test_export_is_lazy_and_not_in_all():
    assert "BinaryGallery" not in M.__all__
    assert M.BinaryGallery is binary.BinaryGallery
