"""int8 resident gallery, the parts that need no GPU: the C-ABI symbols, argument checks (rejected before any HIP call, with a
message), buffer and workspace sizes, and the Python-side checks."""
import ctypes

import pytest
import torch

from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, Int8Gallery, MI355Error, _lib

NEW = ["mi355_gallery_i8_bytes", "mi355_gallery_to_i8", "mi355_rank_i8_workspace_bytes", "mi355_rank_topk_i8",
       "mi355_rank_topk_i8_filtered", "mi355_range_i8_workspace_bytes", "mi355_cosine_range_i8"]


def test_symbols_declared_bound_and_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert L.mi355_abi_version() == 3


def test_buffer_bytes_use_the_padded_stride():
    L = _lib.lib()
    assert L.mi355_gallery_i8_bytes(10, 70) == 1280                   # D = 70 is charged 128 bytes per row
    assert L.mi355_gallery_i8_bytes(3, 1536) == 4608                  # no padding at D = 1536
    assert L.mi355_gallery_i8_bytes(1, 1) == 128
    assert L.mi355_gallery_i8_bytes(2, 128) == 256
    assert L.mi355_gallery_i8_bytes(2, 129) == 512
    assert L.mi355_gallery_i8_bytes(0, 512) == 0
    assert L.mi355_gallery_i8_bytes(5, 0) == 0


def test_workspace_sizes():
    L = _lib.lib()
    assert 0 < L.mi355_rank_i8_workspace_bytes(256, 100000, 1536, 3) < 16 * 2**20    # k <= 8: no score slab
    assert 0 < L.mi355_rank_i8_workspace_bytes(256, 100000, 1536, 8) < 16 * 2**20
    assert L.mi355_rank_i8_workspace_bytes(256, 100000, 1536, 150) > 256 * 100000 * 4
    assert L.mi355_rank_i8_workspace_bytes(1, 100000, 70, 1024) > 100000 * 4
    assert L.mi355_rank_i8_workspace_bytes(0, 10, 8, 1) == 0
    assert L.mi355_rank_i8_workspace_bytes(4, 10, 0, 1) == 0
    assert L.mi355_rank_i8_workspace_bytes(4, 10, 8, 0) == 0
    assert L.mi355_rank_i8_workspace_bytes(4, 2000, 8, 1025) == 0
    assert L.mi355_rank_i8_workspace_bytes(4, 2000, 65537, 1) == 0
    assert L.mi355_range_i8_workspace_bytes(256, 100000, 1536) > 0
    assert L.mi355_range_i8_workspace_bytes(-1, 10, 8) == 0
    assert L.mi355_range_i8_workspace_bytes(4, 10, 0) == 0
    assert L.mi355_range_i8_workspace_bytes(4, 10, 65537) == 0


def _err():
    return _lib.lib().mi355_last_error()


def test_conversion_argument_errors():
    L = _lib.lib()

    def call(rows=4096, G=4, dim=8, codes=4096, codes_bytes=1024, scales=8192):
        return L.mi355_gallery_to_i8(rows, G, dim, 0, 1e-6, codes, codes_bytes, scales, None)

    assert call(rows=None) != 0 and b"null" in _err()
    assert call(codes=None) != 0 and b"null" in _err()
    assert call(scales=None) != 0 and b"null" in _err()
    assert call(dim=0) != 0 and b"bad shape" in _err()
    assert call(G=-1) != 0 and b"bad shape" in _err()
    assert call(dim=65537, codes_bytes=1 << 40) != 0 and b"exceeds 65536" in _err()
    assert call(codes=4104) != 0 and b"16-byte aligned" in _err()
    assert call(dim=70, codes_bytes=4 * 70) != 0 and b"output buffer" in _err()      # the stride is 128, not 70


def test_search_argument_errors():
    L = _lib.lib()
    filt = _lib.RankFilter()

    def plain(q=4096, Q=8, g=8192, s=12288, G=100, dim=64, k=3, out_val=16384, out_idx=32768, ws=65536, ws_bytes=1 << 40):
        return L.mi355_rank_topk_i8(q, Q, g, s, G, dim, k, 1e-6, 0, out_val, out_idx, ws, ws_bytes, None)

    def filtered(f=ctypes.byref(filt), q=4096, Q=8, g=8192, s=12288, G=100, dim=64, k=3, out_val=16384, out_idx=32768, ws=65536,
                 ws_bytes=1 << 40):
        return L.mi355_rank_topk_i8_filtered(q, Q, g, s, G, dim, k, 1e-6, 0, f, out_val, out_idx, ws, ws_bytes, None)

    for call in (plain, filtered):
        assert call(q=None) != 0 and b"null" in _err()
        assert call(g=None) != 0 and b"null" in _err()
        assert call(s=None) != 0 and b"null" in _err()
        assert call(out_idx=None) != 0 and b"null" in _err()
        assert call(dim=0) != 0 and b"bad shape" in _err()
        assert call(G=0) != 0 and b"bad shape" in _err()
        assert call(Q=-1) != 0 and b"bad shape" in _err()
        assert call(dim=65537) != 0 and b"exceeds 65536" in _err()
        assert call(k=0) != 0 and b"outside" in _err()
        assert call(k=101) != 0 and b"outside" in _err()
        assert call(G=5000, k=1025) != 0 and b"outside" in _err()
        assert call(g=8200) != 0 and b"16-byte aligned" in _err()
        assert call(ws_bytes=1024) != 0 and b"workspace" in _err()
        assert call(ws=None) != 0 and b"workspace" in _err()
    assert filtered(f=None) != 0 and b"null filter" in _err()


def test_range_argument_errors():
    L = _lib.lib()
    nnz = ctypes.c_int64(0)

    def call(q=4096, Q=8, g=8192, s=12288, G=100, dim=64, thr=0.5, cand=1 << 20, cap=1024, n=ctypes.byref(nnz), ws=65536,
             ws_bytes=1 << 40):
        return L.mi355_cosine_range_i8(q, Q, g, s, G, dim, 1e-6, thr, 0, None, cand, cap, n, ws, ws_bytes, None)

    assert call(q=None) != 0 and b"null" in _err()
    assert call(g=None) != 0 and b"null" in _err()
    assert call(s=None) != 0 and b"null" in _err()
    assert call(dim=0) != 0 and _err()
    assert call(dim=65537) != 0 and b"exceeds 65536" in _err()
    assert call(thr=float("nan")) != 0 and _err()
    assert call(g=8200) != 0 and b"16-byte aligned" in _err()
    assert call(ws_bytes=1024) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()


def test_gallery_still_rejects_int8_and_the_new_class_checks_its_dim():
    with pytest.raises(MI355Error):
        Gallery(16, "cpu", dtype=torch.int8)
    with pytest.raises(MI355Error):
        Int8Gallery(0, "cpu")
    with pytest.raises(MI355Error):
        Int8Gallery(65537, "cpu", capacity=1 << 40)                   # would not fit anywhere: the check comes first
