"""Asymmetric binary search, the parts that need no GPU: the C-ABI symbols, every argument check of the new entries (rejected
before any HIP call, with a message), the sizer and the Python-side checks."""
import ctypes

import pytest
import torch

from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib, binary

NEW = ["mi355_binary_asym_search_workspace_bytes", "mi355_binary_asym_search", "mi355_binary_asym_distances",
       "mi355_binary_asym_query_codes"]
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
    # the same argument lists as the symmetric entries
    assert _lib.PROTOTYPES["mi355_binary_asym_search"] == _lib.PROTOTYPES["mi355_binary_search"]
    assert _lib.PROTOTYPES["mi355_binary_asym_distances"] == _lib.PROTOTYPES["mi355_binary_distances"]


def test_sizer():
    s = _lib.lib().mi355_binary_asym_search_workspace_bytes
    assert s(0, 1000, 64, 3) == 0 and s(0, 1000, 64, 0) == 0                          # Q = 0
    for k in (0, 3, 150):                                                             # monotone in Q, G and dim
        assert 0 < s(1, 1000, 1536, k) <= s(16, 1000, 1536, k) <= s(256, 1000, 1536, k) <= s(1000, 1000, 1536, k)
        assert s(16, 1000, 1536, k) <= s(16, 100000, 1536, k) <= s(16, 1000000, 1536, k)
        assert s(16, 1000, 64, k) <= s(16, 1000, 1536, k) <= s(16, 1000, 2560, k)
    assert s(256, 1000000, 1536, 3) < 64 << 20                                        # k <= 8: candidates, no slab
    assert s(256, 1000000, 1536, 150) < 256 << 20                                     # k > 8: 8 per chunk + 18 chunks, no slab
    assert 256 * 1536 <= s(256, 100000, 1536, 0) < 1 << 20                            # distances: the queries' int8 codes only
    assert 32 * 1536 <= s(1, 100000, 1536, 0)                                         # whole tiles of 32 queries
    for bad in ((4, 10, 0, 1), (4, 10, 65537, 1), (4, 10, 64, 1025), (4, 10, 64, -1), (4, -1, 64, 1), (-1, 10, 64, 1),
                (4, 1 << 31, 64, 1), (1 << 31, 10, 64, 1)):
        assert s(*bad) == 0, bad


def test_distances_and_search_argument_errors():
    L = _lib.lib()
    filt = _lib.RankFilter()

    def distances(q=4096, Q=8, dim=64, center=8192, codes=16384, G=100, out=32768, ws=65536, ws_bytes=BIG):
        return L.mi355_binary_asym_distances(q, Q, dim, 1e-6, center, codes, G, out, ws, ws_bytes, None)

    def search(q=4096, Q=8, dim=64, center=8192, codes=16384, G=100, k=3, f=None, out=32768, out_idx=49152, ws=65536, ws_bytes=BIG):
        return L.mi355_binary_asym_search(q, Q, dim, 1e-6, center, codes, G, k, 0, f, out, out_idx, ws, ws_bytes, None)

    for call, who in ((distances, b"binary_asym_distances"), (search, b"binary_asym_search")):
        for name in ("q", "codes", "out"):
            assert call(**{name: None}) != 0 and b"null" in _err() and who in _err()
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


def test_query_codes_argument_errors():
    L = _lib.lib()

    def call(q=4096, Q=8, dim=64, center=8192, codes=16384, l1=32768, nan=49152):
        return L.mi355_binary_asym_query_codes(q, Q, dim, 1e-6, center, codes, l1, nan, None)

    for name in ("q", "codes", "l1", "nan"):
        assert call(**{name: None}) != 0 and b"null" in _err() and b"binary_asym_query_codes" in _err()
    assert call(Q=-1) != 0 and b"bad shape" in _err()
    assert call(dim=0) != 0 and b"bad shape" in _err()
    assert call(dim=65537) != 0 and b"exceeds 65536" in _err()
    assert call(Q=1 << 31) != 0 and b"too large" in _err()
    assert call(Q=0) == 0 and call(Q=0, center=None) == 0                             # nothing to do


def test_asymmetric_must_be_a_bool():
    g = binary.BinaryGallery(64, "cpu")
    g.rows = 500                                                                      # as if rows had been added
    q = torch.zeros(2, 64)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(MI355Error, match="asymmetric must be a bool"):
            g.search(q, 3, asymmetric=bad)
        with pytest.raises(MI355Error, match="asymmetric must be a bool"):
            g.distances(q, asymmetric=bad)
    for call in (lambda x: g.search(x, 3, asymmetric=True), lambda x: g.distances(x, asymmetric=True), g.query_codes):
        with pytest.raises(MI355Error, match="queries must live on the GPU"):
            call(q)
    with pytest.raises(MI355Error, match="k out of range"):
        g.search(q, 501, asymmetric=True)
