"""Ranking metrics without a GPU: the new C symbols, every argument check of the new entries (each refused before any HIP call,
with a message) and the Python-side checks, which run before anything is asked of a device."""
import ctypes as C

import pytest
import torch

from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib
from imageretrievalresearch_amd import rank as R
import imageretrievalresearch_amd as M

NEW = ["mi355_positives_range", "mi355_positives_range_f16", "mi355_rank_positives_keys", "mi355_rank_positives_workspace_bytes",
       "mi355_rank_positives", "mi355_rank_positives_f16_workspace_bytes", "mi355_rank_positives_f16",
       "mi355_rank_positives_finalize"]
FAKE = C.c_void_p(4096)          # never dereferenced: every call below fails its argument checks first


def _i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_stays_3():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name
    assert _lib.lib().mi355_abi_version() == 3
    for name in ("positive_ranks", "ranking_metrics", "PositiveRanks"):
        assert name in M.__all__ and hasattr(M, name)


def _count(q=FAKE, g=FAKE, ql=FAKE, gl=FAKE, off=FAKE, off_host=None, keys=FAKE, nnz=5, before=FAKE, block=0, Q=8, G=100, dim=64,
           ws=FAKE, wsb=1 << 40):
    return _lib.lib().mi355_rank_positives(q, Q, g, G, dim, 0, 1e-6, ql, gl, None, 0, off, off_host, keys, nnz, before, block, ws,
                                           wsb, None)


def _count16(q=FAKE, g=FAKE, ql=FAKE, gl=FAKE, off=FAKE, off_host=None, keys=FAKE, nnz=5, before=FAKE, block=0, Q=8, G=100, dim=64,
             ws=FAKE, wsb=1 << 40):
    return _lib.lib().mi355_rank_positives_f16(q, Q, g, G, dim, 1e-6, ql, gl, None, 0, off, off_host, keys, nnz, before, block, ws,
                                               wsb, None)


@pytest.mark.parametrize("entry", [_count, _count16], ids=["fp32", "f16"])
def test_counting_pass_checks(entry):
    L = _lib.lib()
    good = _i64([0, 1, 1, 2, 3, 3, 4, 5, 5])
    cases = [
        (dict(q=None), b"null queries/gallery"),
        (dict(g=None), b"null queries/gallery"),
        (dict(ql=None), b"null query_labels/gallery_labels"),
        (dict(gl=None), b"null query_labels/gallery_labels"),
        (dict(off=None), b"null offsets"),
        (dict(Q=0), b"bad shape"),
        (dict(G=0), b"bad shape"),
        (dict(dim=0), b"bad shape"),
        (dict(Q=1 << 31), b"shape too large"),
        (dict(G=(1 << 31) - 128), b"shape too large"),
        (dict(G=1 << 31), b"shape too large"),
        (dict(nnz=-1), b"nnz=-1"),
        (dict(nnz=801), b"nnz=801"),
        (dict(keys=None), b"null pos_keys/before"),
        (dict(before=None), b"null pos_keys/before"),
        (dict(keys=C.c_void_p(4100)), b"8-byte aligned"),
        (dict(block=-1), b"query_block=-1"),
        (dict(off_host=_i64([1, 1, 1, 2, 3, 3, 4, 5, 5])), b"offsets[0] = 1"),
        (dict(off_host=_i64([0, 2, 1, 2, 3, 3, 4, 5, 5])), b"monotone"),
        (dict(off_host=_i64([0, 0, 0, 0, 0, 0, 0, 0, 101]), nnz=101), b"at most G per query"),
        (dict(off_host=good, nnz=4), b"offsets[Q] = 5 but nnz = 4"),
        (dict(off_host=good, ws=None), b"workspace"),
        (dict(off_host=good, wsb=16), b"workspace"),
    ]
    for kw, msg in cases:
        assert entry(**kw) != 0, kw
        assert msg in L.mi355_last_error(), (kw, msg, L.mi355_last_error())
    if entry is _count16:
        assert entry(g=C.c_void_p(4104)) != 0 and b"16-byte aligned" in L.mi355_last_error()


def test_positives_range_keys_and_finalize_checks():
    L = _lib.lib()
    nnz = C.c_int64(0)
    same = _lib.RankFilter()
    same.label_mode = _lib.LABEL_SAME
    anyf = _lib.RankFilter()
    for filt, msg in ((None, b"needs a filter"), (C.byref(anyf), b"needs a filter"), (C.byref(same), b"label")):
        assert L.mi355_positives_range(FAKE, 8, FAKE, 100, 64, 0, 1e-6, 0, filt, FAKE, 16, C.byref(nnz), FAKE, 1 << 40, None) != 0
        assert msg in L.mi355_last_error(), (msg, L.mi355_last_error())
        assert L.mi355_positives_range_f16(FAKE, 8, FAKE, 100, 64, 1e-6, 0, filt, FAKE, 16, C.byref(nnz), FAKE, 1 << 40, None) != 0
        assert msg in L.mi355_last_error(), (msg, L.mi355_last_error())
    same.query_labels, same.gallery_labels = 4096, 4096
    assert L.mi355_positives_range(None, 8, FAKE, 100, 64, 0, 1e-6, 0, C.byref(same), FAKE, 16, C.byref(nnz), FAKE, 1 << 40, None) != 0
    assert b"null queries/gallery" in L.mi355_last_error()
    assert L.mi355_positives_range(FAKE, 8, FAKE, 1 << 31, 64, 0, 1e-6, 0, C.byref(same), FAKE, 16, C.byref(nnz), FAKE, 1 << 40, None) != 0
    assert b"shape too large" in L.mi355_last_error()
    assert L.mi355_positives_range(FAKE, 8, FAKE, 100, 64, 0, 1e-6, 0, C.byref(same), FAKE, 16, C.byref(nnz), FAKE, 16, None) != 0
    assert b"workspace" in L.mi355_last_error()
    # keys
    assert L.mi355_rank_positives_keys(FAKE, FAKE, -1, 0, FAKE, None) != 0 and b"nnz=-1" in L.mi355_last_error()
    for p in range(3):
        args = [FAKE] * 3
        args[p] = None
        assert L.mi355_rank_positives_keys(args[0], args[1], 4, 0, args[2], None) != 0 and b"null" in L.mi355_last_error()
    assert L.mi355_rank_positives_keys(None, None, 0, 0, None, None) == 0          # nothing to do
    # finalize
    assert L.mi355_rank_positives_finalize(FAKE, FAKE, 0, 4, FAKE, FAKE, FAKE, None) != 0 and b"Q=0" in L.mi355_last_error()
    assert L.mi355_rank_positives_finalize(FAKE, FAKE, 8, -1, FAKE, FAKE, FAKE, None) != 0 and b"nnz=-1" in L.mi355_last_error()
    for args in ((None, FAKE, FAKE, FAKE, FAKE), (FAKE, FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, FAKE, None)):
        assert L.mi355_rank_positives_finalize(args[0], args[1], 8, 4, *args[2:], None) != 0
        assert b"null offsets/ap/first_rank" in L.mi355_last_error()
    for args in ((FAKE, None, FAKE, FAKE, FAKE), (FAKE, FAKE, None, FAKE, FAKE)):
        assert L.mi355_rank_positives_finalize(args[0], args[1], 8, 4, *args[2:], None) != 0
        assert b"null before/ranks" in L.mi355_last_error()


def test_workspace_has_no_pair_term():
    L = _lib.lib()
    assert L.mi355_rank_positives_workspace_bytes(100000, 100000, 1536) < 100000 * 1536 * 4 + 256 * 2**20
    assert L.mi355_rank_positives_f16_workspace_bytes(100000, 100000, 1536) < 100000 * 1536 * 4 + 256 * 2**20
    assert L.mi355_rank_positives_workspace_bytes(0, 10, 8) == 0 and L.mi355_rank_positives_f16_workspace_bytes(4, 10, 0) == 0


def test_python_argument_errors_come_before_any_device_work():
    q, ql = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    g, gl = torch.zeros(6, 8), torch.zeros(6, dtype=torch.int64)
    for fn in (M.ranking_metrics, M.positive_ranks):
        with pytest.raises(MI355Error, match=r"query_labels must have shape \(4,\)"):
            fn(q, ql[:3], g, gl)
        with pytest.raises(MI355Error, match=r"query_labels must have shape \(4,\)"):
            fn(q, ql[:3])
        with pytest.raises(MI355Error, match=r"gallery_labels must have shape \(6,\)"):
            fn(q, ql, g, gl[:5])
        with pytest.raises(MI355Error, match=r"gallery_labels must have shape \(6,\)"):
            fn(q, ql, g, torch.zeros(6, 1, dtype=torch.int64))
        with pytest.raises(MI355Error, match="gallery_labels given without a gallery"):
            fn(q, ql, None, gl)
        with pytest.raises(MI355Error, match="a gallery needs gallery_labels"):
            fn(q, ql, g)
        with pytest.raises(MI355Error, match=r"Q=0"):
            fn(q[:0], ql[:0], g, gl)
        with pytest.raises(MI355Error, match=r"G=0"):
            fn(q, ql, g[:0], gl[:0])
        with pytest.raises(MI355Error, match=r"at least one other gallery row \(Q=1, G=1\)"):
            fn(q[:1], ql[:1])
        with pytest.raises(MI355Error, match="embedding dims differ"):
            fn(q, ql, torch.zeros(6, 9), gl)
        with pytest.raises(MI355Error, match=r"queries must be \(Q, D\)"):
            fn(torch.zeros(4), ql, g, gl)
        with pytest.raises(MI355Error, match="queries on cpu but gallery on meta"):
            fn(q, ql, torch.zeros(6, 8, device="meta"), gl)
        with pytest.raises(MI355Error, match="must be a tensor"):
            fn(q, [0, 1, 2, 3], g, gl)
        with pytest.raises(MI355Error, match="must live on the GPU"):      # nothing else is wrong with these
            fn(q, ql, g, gl)
    for bad in ((0,), (1, -5), (1.5,), (), (True,), 5, ("1",)):
        with pytest.raises(MI355Error, match="ranks must be"):
            M.ranking_metrics(q, ql, g, gl, ranks=bad)
    with pytest.raises(MI355Error, match="same-source"):
        M.positive_ranks(q, ql, exclude=ql)
    with pytest.raises(MI355Error, match="same-source"):
        M.positive_ranks(q, ql, idx_offset=3)
    assert R._cmc_ranks((20, 1, 5, 5)) == [1, 5, 20]


def test_gallery_method_errors_without_a_device():
    q, ql = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    gal = R.Gallery(8, "cpu")
    with pytest.raises(MI355Error, match="needs gallery labels"):
        gal.ranking_metrics(q, ql)
    gal.labels, gal.rows = torch.zeros(6, dtype=torch.int64), 6        # (no row can be added without a device)
    gal._buf = torch.zeros(6, 8)
    with pytest.raises(MI355Error, match=r"query_labels must have shape \(4,\)"):
        gal.ranking_metrics(q, ql[:2])
    with pytest.raises(MI355Error, match="embedding dims differ"):
        gal.ranking_metrics(torch.zeros(4, 9), ql)
    with pytest.raises(MI355Error, match="ranks must be"):
        gal.ranking_metrics(q, ql, ranks=(0,))
    with pytest.raises(MI355Error, match="must live on the GPU"):
        gal.ranking_metrics(q, ql)
