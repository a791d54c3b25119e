"""fp16 resident gallery, the parts that need no GPU: the C-ABI symbols, argument checks (rejected before any HIP call, with a
message), buffer and workspace sizes, and the Python-side dtype checks."""
import ctypes

import pytest
import torch

from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, MI355Error, _lib
from imageretrievalresearch_amd.sharded import ShardedGallery

NEW = ["mi355_gallery_f16_bytes", "mi355_gallery_to_f16", "mi355_rank_f16_workspace_bytes", "mi355_rank_topk_f16"]


def test_symbols_declared_bound_and_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert L.mi355_abi_version() == 3


def test_buffer_bytes_use_the_padded_stride():
    L = _lib.lib()
    assert L.mi355_gallery_f16_bytes(10, 70) == 10 * 128 * 2          # D = 70 is charged 128 elements per row
    assert L.mi355_gallery_f16_bytes(3, 1536) == 3 * 1536 * 2         # no padding at D = 1536
    assert L.mi355_gallery_f16_bytes(1, 1) == 64 * 2
    assert L.mi355_gallery_f16_bytes(2, 64) == 2 * 64 * 2
    assert L.mi355_gallery_f16_bytes(2, 65) == 2 * 128 * 2
    assert L.mi355_gallery_f16_bytes(0, 512) == 0
    assert L.mi355_gallery_f16_bytes(5, 0) == 0


def test_workspace_sizes():
    L = _lib.lib()
    assert L.mi355_rank_f16_workspace_bytes(256, 100000, 1536, 3) < 16 * 2**20       # k <= 8: no score slab
    assert L.mi355_rank_f16_workspace_bytes(256, 100000, 1536, 150) > 256 * 100000 * 4
    assert L.mi355_rank_f16_workspace_bytes(1, 100000, 70, 1024) > 100000 * 4
    assert L.mi355_rank_f16_workspace_bytes(0, 10, 8, 1) == 0
    assert L.mi355_rank_f16_workspace_bytes(4, 10, 0, 1) == 0
    assert L.mi355_rank_f16_workspace_bytes(4, 10, 8, 0) == 0
    assert L.mi355_rank_f16_workspace_bytes(4, 2000, 8, 1025) == 0


def _err():
    return _lib.lib().mi355_last_error()


def test_conversion_argument_errors():
    L = _lib.lib()
    assert L.mi355_gallery_to_f16(None, 4, 8, 0, 1e-6, 4096, 1024, None) != 0
    assert b"null" in _err()
    assert L.mi355_gallery_to_f16(4096, 4, 0, 0, 1e-6, 4096, 1024, None) != 0
    assert b"bad shape" in _err()
    assert L.mi355_gallery_to_f16(4096, -1, 8, 0, 1e-6, 4096, 1024, None) != 0
    assert b"bad shape" in _err()
    assert L.mi355_gallery_to_f16(4096, 4, 8, 0, 1e-6, 4104, 1024, None) != 0
    assert b"16-byte aligned" in _err()
    assert L.mi355_gallery_to_f16(4096, 4, 70, 0, 1e-6, 4096, 4 * 70 * 2, None) != 0     # the stride is 128, not 70
    assert b"output buffer" in _err()


def test_search_argument_errors():
    L = _lib.lib()

    def call(q=4096, Q=8, g=8192, G=100, dim=64, k=3, out_val=16384, out_idx=32768, ws=65536, ws_bytes=1 << 40):
        return L.mi355_rank_topk_f16(q, Q, g, G, dim, k, 1e-6, 0, out_val, out_idx, ws, ws_bytes, None)

    assert call(q=None) != 0 and b"null" in _err()
    assert call(g=None) != 0 and b"null" in _err()
    assert call(out_idx=None) != 0 and b"null" in _err()
    assert call(dim=0) != 0 and b"bad shape" in _err()
    assert call(G=0) != 0 and b"bad shape" in _err()
    assert call(Q=-1) != 0 and b"bad shape" in _err()
    assert call(k=0) != 0 and b"outside" in _err()
    assert call(k=101) != 0 and b"outside" in _err()
    assert call(G=5000, k=1025) != 0 and b"outside" in _err()
    assert call(g=8200) != 0 and b"16-byte aligned" in _err()
    assert call(ws_bytes=1024) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()


def test_gallery_rejects_other_dtypes_before_allocating():
    for dt in (torch.int8, torch.bfloat16, torch.float64):
        with pytest.raises(MI355Error):
            Gallery(16, "cpu", capacity=1 << 40, dtype=dt)        # would not fit anywhere: the check comes first


def test_sharded_gallery_dtype_checks():
    rows = torch.zeros(3, 8)
    with pytest.raises(MI355Error):
        ShardedGallery(rows, dtype=torch.int8)
    with pytest.raises(MI355Error):
        ShardedGallery(rows, prepared=True, dtype=torch.float16)
