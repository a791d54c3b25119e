"""fp4 resident gallery, the parts that need no GPU: the C-ABI symbols, argument checks (rejected before any HIP call, with a
message), buffer and workspace sizes, and the Python-side checks."""
import ctypes

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, Int8Gallery, MI355Error, _lib
from imageretrievalresearch_amd.fp4 import FP4Gallery

NEW = ["mi355_gallery_fp4_bytes", "mi355_gallery_to_fp4", "mi355_rank_fp4_workspace_bytes", "mi355_rank_topk_fp4",
       "mi355_rank_topk_fp4_filtered", "mi355_range_fp4_workspace_bytes", "mi355_cosine_range_fp4"]


def test_symbols_declared_bound_and_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert L.mi355_abi_version() == 3


def test_exported_lazily_and_kept_out_of_the_stream_table():
    assert M.FP4Gallery is FP4Gallery
    assert "FP4Gallery" not in M.__all__


def test_buffer_bytes_use_the_padded_stride():
    L = _lib.lib()
    assert L.mi355_gallery_fp4_bytes(10, 70) == 1280                  # 35 bytes of codes are charged 128 per row
    assert L.mi355_gallery_fp4_bytes(3, 1536) == 3 * 768              # no padding at D = 1536: 772 B a row with its multiplier
    assert L.mi355_gallery_fp4_bytes(1, 1) == 128
    assert L.mi355_gallery_fp4_bytes(2, 256) == 256
    assert L.mi355_gallery_fp4_bytes(2, 257) == 512                   # the odd dimension takes a byte of its own
    assert L.mi355_gallery_fp4_bytes(1, 65536) == 32768
    assert L.mi355_gallery_fp4_bytes(0, 512) == 0
    assert L.mi355_gallery_fp4_bytes(5, 0) == 0


def test_workspace_sizes():
    L = _lib.lib()
    assert 0 < L.mi355_rank_fp4_workspace_bytes(256, 100000, 1536, 3) < 16 * 2**20   # k <= 8: no score slab
    assert 0 < L.mi355_rank_fp4_workspace_bytes(256, 100000, 1536, 8) < 16 * 2**20
    assert L.mi355_rank_fp4_workspace_bytes(256, 100000, 1536, 150) > 256 * 100000 * 4
    assert L.mi355_rank_fp4_workspace_bytes(1, 100000, 70, 1024) > 100000 * 4
    # the planes are half those of the int8 search
    assert L.mi355_rank_fp4_workspace_bytes(256, 100000, 1536, 3) < L.mi355_rank_i8_workspace_bytes(256, 100000, 1536, 3)
    assert L.mi355_rank_fp4_workspace_bytes(0, 10, 8, 1) == 0
    assert L.mi355_rank_fp4_workspace_bytes(4, 10, 0, 1) == 0
    assert L.mi355_rank_fp4_workspace_bytes(4, 10, 8, 0) == 0
    assert L.mi355_rank_fp4_workspace_bytes(4, 2000, 8, 1025) == 0
    assert L.mi355_rank_fp4_workspace_bytes(4, 2000, 65537, 1) == 0
    assert L.mi355_rank_fp4_workspace_bytes(4, 2000, 65536, 1) > 0
    assert L.mi355_range_fp4_workspace_bytes(256, 100000, 1536) > 0
    assert L.mi355_range_fp4_workspace_bytes(-1, 10, 8) == 0
    assert L.mi355_range_fp4_workspace_bytes(4, 10, 0) == 0
    assert L.mi355_range_fp4_workspace_bytes(4, 10, 65537) == 0


def _err():
    return _lib.lib().mi355_last_error()


def test_conversion_argument_errors():
    L = _lib.lib()

    def call(rows=4096, G=4, dim=8, codes=4096, codes_bytes=1024, mults=8192):
        return L.mi355_gallery_to_fp4(rows, G, dim, 0, 1e-6, codes, codes_bytes, mults, None)

    assert call(rows=None) != 0 and b"null" in _err()
    assert call(codes=None) != 0 and b"null" in _err()
    assert call(mults=None) != 0 and b"null" in _err()
    assert call(dim=0) != 0 and b"bad shape" in _err()
    assert call(G=-1) != 0 and b"bad shape" in _err()
    assert call(dim=65537, codes_bytes=1 << 40) != 0 and b"exceeds 65536" in _err()
    assert call(codes=4104) != 0 and b"16-byte aligned" in _err()
    assert call(dim=70, codes_bytes=4 * 35) != 0 and b"output buffer" in _err()      # the stride is 128, not 35
    assert call(G=0, codes_bytes=0) == 0                                             # nothing to convert: no launch


def test_search_argument_errors():
    L = _lib.lib()
    filt = _lib.RankFilter()

    def plain(q=4096, Q=8, g=8192, s=12288, G=100, dim=64, k=3, out_val=16384, out_idx=32768, ws=65536, ws_bytes=1 << 40):
        return L.mi355_rank_topk_fp4(q, Q, g, s, G, dim, k, 1e-6, 0, out_val, out_idx, ws, ws_bytes, None)

    def filtered(f=ctypes.byref(filt), q=4096, Q=8, g=8192, s=12288, G=100, dim=64, k=3, out_val=16384, out_idx=32768, ws=65536,
                 ws_bytes=1 << 40):
        return L.mi355_rank_topk_fp4_filtered(q, Q, g, s, G, dim, k, 1e-6, 0, f, out_val, out_idx, ws, ws_bytes, None)

    for call in (plain, filtered):
        assert call(q=None) != 0 and b"null" in _err()
        assert call(g=None) != 0 and b"null" in _err()
        assert call(s=None) != 0 and b"null" in _err()
        assert call(out_val=None) != 0 and b"null" in _err()
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
        assert b"fp4" in _err()                                      # the message names the entry
    assert filtered(f=None) != 0 and b"null filter" in _err()


def test_range_argument_errors():
    L = _lib.lib()
    nnz = ctypes.c_int64(0)

    def call(q=4096, Q=8, g=8192, s=12288, G=100, dim=64, thr=0.5, cand=1 << 20, cap=1024, n=ctypes.byref(nnz), ws=65536,
             ws_bytes=1 << 40):
        return L.mi355_cosine_range_fp4(q, Q, g, s, G, dim, 1e-6, thr, 0, None, cand, cap, n, ws, ws_bytes, None)

    assert call(q=None) != 0 and b"null" in _err()
    assert call(g=None) != 0 and b"null" in _err()
    assert call(s=None) != 0 and b"null" in _err()
    assert call(dim=0) != 0 and _err()
    assert call(dim=65537) != 0 and b"exceeds 65536" in _err()
    assert call(thr=float("nan")) != 0 and _err()
    assert call(g=8200) != 0 and b"16-byte aligned" in _err()
    assert call(ws_bytes=1024) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()


def test_the_class_checks_its_arguments():
    with pytest.raises(MI355Error, match="1 <= dim <= 65536"):
        FP4Gallery(0, "cpu")
    with pytest.raises(MI355Error, match="1 <= dim <= 65536"):
        FP4Gallery(65537, "cpu", capacity=1 << 40)                    # would not fit anywhere: the check comes first
    g = FP4Gallery(257, "cpu", capacity=3)
    assert g._codes.shape == (3, 256) and g._codes.dtype == torch.uint8 and g._mults.shape == (3,)
    assert len(g) == 0 and g.codes.shape == (0, 129) and g.mults.shape == (0,) and g.nbytes == 3 * 260
    assert FP4Gallery(1536, "cpu", capacity=1).nbytes == 772
    q = torch.zeros(1, 257)
    with pytest.raises(MI355Error):
        g.add(torch.zeros(2, 257))                                   # rows on the CPU
    with pytest.raises(MI355Error, match="selected index k out of range"):
        g.search(q, 1, refine=Gallery(257, "cpu"))                   # no rows yet
    g.rows = 3                                                       # the checks below read no row
    with pytest.raises(MI355Error, match="shortlist is the length"):
        g.search(q, 1, shortlist=2)
    with pytest.raises(MI355Error, match="refine holds 0 rows"):
        g.search(q, 1, refine=Gallery(257, "cpu"))
    with pytest.raises(MI355Error, match="shortlist=5 outside"):
        g.search(q, 1, refine=_three_rows(257), shortlist=5)
    with pytest.raises(MI355Error, match="needs gallery labels"):
        g.search(q, 1, query_labels=torch.zeros(1), label_filter="same")
    with pytest.raises(MI355Error, match="needs gallery labels"):
        g.range_search(q, 0.5, query_labels=torch.zeros(1), label_filter="same")
    with pytest.raises(MI355Error, match="recall needs a Gallery"):
        g.recall(q, 1, Int8Gallery(257, "cpu"))
    with pytest.raises(MI355Error, match="fp32 rows of a Gallery"):
        FP4Gallery.from_gallery(Int8Gallery(16, "cpu"))
    with pytest.raises(MI355Error, match="fp32 rows of a Gallery"):
        FP4Gallery.from_gallery(Gallery(16, "cpu", dtype=torch.float16))


def _three_rows(dim):
    g = Gallery(dim, "cpu", capacity=3)
    g.rows = 3
    return g


def test_what_rejects_an_int8_gallery_by_type_rejects_this_one():
    g = FP4Gallery(16, "cpu", capacity=3)
    g.rows = 3
    store = Int8Gallery(16, "cpu", capacity=3)
    store.rows = 3
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        store.search(torch.zeros(1, 16), 1, refine=g)
    with pytest.raises(MI355Error, match="recall needs a Gallery"):
        store.recall(torch.zeros(1, 16), 1, g)
    with pytest.raises(MI355Error, match="built over an Int8Gallery"):
        M.Int8IVFIndex(g, torch.zeros(1, 16), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(MI355Error, match="Gallery dtype"):
        Gallery(16, "cpu", dtype=torch.uint8)
