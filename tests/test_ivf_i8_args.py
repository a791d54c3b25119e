"""IVF search over an int8 gallery, the parts that need no GPU: the C-ABI symbols, every argument check of the new entry
(rejected before any HIP call, with a message), the workspace sizes, the Python-side checks, the export, and the NumPy model of
the index against the model of the exhaustive search."""
import ctypes

import numpy as np
import pytest
import torch

import gallery_i8_ref as R8
import imageretrievalresearch_amd as M
import ivf_i8_ref as R
import ivf_ref as I
from helpers import header_symbols
from imageretrievalresearch_amd import Gallery, Int8Gallery, MI355Error, _lib, ivf_i8

NEW = ["mi355_ivf_scan_i8_workspace_bytes", "mi355_ivf_scan_i8"]
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
    s = _lib.lib().mi355_ivf_scan_i8_workspace_bytes            # (Q, nprobe, nlist, dim, cap)
    assert s(0, 8, 256, 1536, 5000) == 0                                              # Q = 0
    assert 0 < s(1, 8, 256, 1536, 5000) <= s(16, 8, 256, 1536, 5000) <= s(256, 8, 256, 1536, 5000) <= s(1000, 8, 256, 1536, 5000)
    assert s(16, 8, 256, 1536, 1000) <= s(16, 8, 256, 1536, 5000) <= s(16, 8, 256, 1536, 100000)
    assert s(16, 8, 256, 70, 5000) <= s(16, 8, 256, 1536, 5000) <= s(16, 8, 256, 4100, 5000) <= s(16, 8, 256, 32768, 5000)
    # the query side is two planes of ld bytes and s_q, half of the fp32 entry's normalised rows
    f = _lib.lib().mi355_ivf_scan_workspace_bytes
    assert 0 < f(256, 8, 256, 1536, 5000) - s(256, 8, 256, 1536, 5000) <= 256 * 1536 * 2
    for bad in ((-1, 8, 256, 64, 100), (4, 0, 256, 64, 100), (4, 257, 256, 64, 100), (4, 8, 0, 64, 100), (4, 8, 1 << 24, 64, 100),
                (4, 8, 256, 0, 100), (4, 8, 256, -1, 100), (4, 8, 256, 65537, 100), (4, 8, 256, 32769, 100), (4, 8, 256, 64, 0),
                (1 << 29, 8, 256, 64, 100), (1 << 20, 1, 256, 64, (1 << 20) + 1)):
        assert s(*bad) == 0, bad


def test_scan_argument_errors():
    L = _lib.lib()
    filt = _lib.RankFilter()

    def call(q=4096, Q=8, dim=64, codes=8192, scales=12288, ld=128, G=1000, offsets=20480, order=24576, nlist=16, probes=28672,
             nprobe=4, cap=500, f=None, out=32768, out_idx=49152, ws=65536, ws_bytes=BIG):
        return L.mi355_ivf_scan_i8(q, Q, dim, 1e-6, codes, scales, ld, G, offsets, order, nlist, probes, nprobe, cap, 0, f, out,
                                   out_idx, ws, ws_bytes, None)

    for name in ("q", "codes", "scales", "offsets", "order", "probes", "out", "out_idx"):
        assert call(**{name: None}) != 0 and b"null" in _err(), name
    assert call(Q=-1) != 0 and b"Q=-1 must be >= 0" in _err()
    for dim in (0, -1, 65537):
        assert call(dim=dim, ld=1 << 17) != 0 and b"outside [1, 65536]" in _err(), dim
    assert call(dim=32769, ld=32896) != 0 and b"too large: one query of 65792 bytes does not fit in 65536 bytes of LDS" in _err()
    assert call(dim=65536, ld=65536) != 0 and b"does not fit" in _err()
    assert call(G=0) != 0 and b"G=0 must be >= 1" in _err()
    for ld in (64, 100, 129, 192, 0, -128):
        assert call(ld=ld) != 0 and b"must be a multiple of 128 and >= dim=64" in _err(), ld
    assert call(dim=130, ld=128) != 0 and b"must be a multiple of 128 and >= dim=130" in _err()
    assert call(codes=8200) != 0 and b"16-byte aligned" in _err()
    for nlist in (0, -1, 1 << 24):
        assert call(nlist=nlist) != 0 and b"nlist=" in _err() and b"outside [1, 2^24)" in _err()
    for nprobe in (0, -1, 17):
        assert call(nprobe=nprobe) != 0 and b"nprobe=" in _err() and b"outside [1, nlist=16]" in _err()
    assert call(cap=0) != 0 and b"cap=0 must be >= 1" in _err()
    assert call(Q=1 << 29, nprobe=4) != 0 and b"too large" in _err()                  # Q * nprobe >= 2^31
    assert call(Q=1 << 20, nprobe=1, cap=(1 << 20) + 1) != 0 and b"too large" in _err()   # Q * cap > 2^40
    filt.label_mode = 7
    assert call(f=ctypes.byref(filt)) != 0 and b"label_mode" in _err()
    filt.label_mode = _lib.LABEL_SAME
    assert call(f=ctypes.byref(filt)) != 0 and b"needs query_labels" in _err()
    assert call(ws_bytes=1024) != 0 and b"workspace" in _err()
    assert call(ws=None) != 0 and b"workspace" in _err()
    need = L.mi355_ivf_scan_i8_workspace_bytes(8, 4, 16, 64, 500)
    assert call(ws_bytes=need - 1) != 0 and b"workspace" in _err()
    assert call(Q=0, ws=None, ws_bytes=0) == 0                                        # nothing to do
    assert call(Q=0, q=None, codes=None, out=None) == 0
    assert call(G=0) != 0 and _err().startswith(b"ivf_scan_i8:")                      # a message names its entry
    # the fp32 / fp16 entry still refuses int8 rows: this is a new entry, not a third dtype of the old one
    assert L.mi355_ivf_scan(4096, 8, 64, 1e-6, 8192, 2, 128, 1000, 20480, 24576, 16, 28672, 4, 500, 0, None, 32768, 49152, 65536,
                            BIG, None) != 0 and b"unknown rows dtype 2" in _err()


def _gallery(dim=64, rows=500, device="cpu"):
    g = Int8Gallery(dim, device)
    g.rows = rows                                                                     # as if rows had been added
    return g


def test_build_checks_its_arguments():
    g = _gallery()
    for cls_call in (lambda store: ivf_i8.Int8IVFIndex.build(store, torch.zeros(500, 64), 4),
                     lambda store: ivf_i8.Int8IVFIndex(store, torch.zeros(4, 64), torch.zeros(500, dtype=torch.int64))):
        with pytest.raises(MI355Error, match="built over an Int8Gallery, got Gallery"):
            cls_call(Gallery(64, "cpu"))
        with pytest.raises(MI355Error, match="at least one row"):
            cls_call(_gallery(rows=0))
        with pytest.raises(MI355Error, match="needs dim <= 32768"):
            cls_call(_gallery(dim=32769))
    with pytest.raises(MI355Error, match="Gallery or a tensor"):
        ivf_i8.Int8IVFIndex.build(g, [[0.0] * 64] * 500, 4)
    with pytest.raises(MI355Error, match="must be fp32"):
        ivf_i8.Int8IVFIndex.build(g, torch.zeros(500, 64, dtype=torch.float16), 4)
    with pytest.raises(MI355Error, match="rows are on meta but the Int8Gallery lives on cpu"):
        ivf_i8.Int8IVFIndex.build(g, torch.zeros(500, 64, device="meta"), 4)
    with pytest.raises(MI355Error, match="rows are on meta"):
        g.ivf(Gallery(64, "meta"), 4)                                                 # the convenience goes the same way
    with pytest.raises(MI355Error, match="rows have dim 32, the Int8Gallery 64"):
        ivf_i8.Int8IVFIndex.build(g, torch.zeros(500, 32), 4)
    with pytest.raises(MI355Error, match=r"\(N, 64\)"):
        ivf_i8.Int8IVFIndex.build(g, torch.zeros(500), 4)
    with pytest.raises(MI355Error, match="rows holds 499 rows, the Int8Gallery 500"):
        ivf_i8.Int8IVFIndex.build(g, torch.zeros(499, 64), 4)
    short = Gallery(64, "cpu")
    short.rows = 499
    with pytest.raises(MI355Error, match="rows holds 499 rows"):
        ivf_i8.Int8IVFIndex.build(g, short, 4)
    with pytest.raises(MI355Error, match=r"centroids must be \(nlist, 64\)"):
        ivf_i8.Int8IVFIndex(g, torch.zeros(4, 32), torch.zeros(500, dtype=torch.int64))
    with pytest.raises(MI355Error, match=r"centroids must be \(nlist, 64\)"):
        ivf_i8.Int8IVFIndex(g, torch.zeros(4, 64, device="meta"), torch.zeros(500, dtype=torch.int64))
    with pytest.raises(MI355Error, match="centroids must be a tensor"):
        ivf_i8.Int8IVFIndex(g, None, torch.zeros(500, dtype=torch.int64))
    with pytest.raises(MI355Error, match="from_gallery needs a Gallery"):
        ivf_i8.Int8IVFIndex.from_gallery(g, 4)


def _index(rows=500, nlist=16):
    """An index as if built, without the GPU: 16 lists of rows // 16 rows (the first takes the remainder)."""
    ix = object.__new__(ivf_i8.Int8IVFIndex)
    ix.i8 = _gallery(rows=rows)
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
    with pytest.raises(MI355Error, match="refine is on meta but the Int8Gallery lives on cpu"):
        ix.search(q, 3, 2, refine=Gallery(64, "meta"))
    other = Gallery(64, "cpu")
    other.rows = 499
    with pytest.raises(MI355Error, match="refine holds 499 rows of dim 64, the Int8Gallery 500 of dim 64"):
        ix.search(q, 3, 2, refine=other)
    wide = Gallery(32, "cpu")
    wide.rows = 500
    with pytest.raises(MI355Error, match="refine holds 500 rows of dim 32"):
        ix.search(q, 3, 2, refine=wide)
    other.rows = 500
    with pytest.raises(MI355Error, match="shortlist=2 outside"):
        ix.search(q, 3, 2, refine=other, shortlist=2)
    with pytest.raises(MI355Error, match="shortlist=501 outside"):
        ix.search(q, 3, 2, refine=other, shortlist=501)
    with pytest.raises(MI355Error, match="give refine too"):
        ix.search(q, 3, 2, shortlist=100)
    with pytest.raises(MI355Error, match="same 500 rows"):
        ix.recall(q, 3, 2, exact=Gallery(64, "cpu"))


def test_the_gallery_search_checks_refine_and_shortlist():
    g = _gallery()
    q = torch.zeros(2, 64)
    with pytest.raises(MI355Error, match="give refine too"):
        g.search(q, 3, shortlist=100)
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        g.search(q, 3, refine=g)
    with pytest.raises(MI355Error, match="refine is on meta but the Int8Gallery lives on cpu"):
        g.search(q, 3, refine=Gallery(64, "meta"))
    other = Gallery(64, "cpu")
    other.rows = 499
    with pytest.raises(MI355Error, match="refine holds 499 rows of dim 64, the Int8Gallery 500 of dim 64"):
        g.search(q, 3, refine=other)
    other.rows = 500
    for short in (2, 501, 1.5):
        with pytest.raises(MI355Error, match="shortlist=.* outside"):
            g.search(q, 3, refine=other, shortlist=short)
    for k in (0, 501):
        with pytest.raises(MI355Error, match="k out of range"):
            g.search(q, k, refine=other)


def test_a_stale_index_refuses_to_search():
    ix = _index()
    assert not ix.stale
    ix.i8.rows = 501                                                                  # as if i8.add had run behind its back
    assert ix.stale
    with pytest.raises(MI355Error, match="stale: it lists 500 rows but the Int8Gallery holds 501 "
                                         r"\(add rows through index.add, or build the index again\)"):
        ix.search(torch.zeros(2, 64), 3, 2)
    with pytest.raises(MI355Error, match="stale"):
        ix.add(torch.zeros(1, 64))


def test_export_is_lazy_and_not_in_all():
    assert "Int8IVFIndex" not in M.__all__
    assert M.Int8IVFIndex is ivf_i8.Int8IVFIndex
    assert "ivf" not in vars(Int8Gallery) and Int8Gallery.ivf is not None            # from a base: no row in the stream table
    assert ivf_i8.Int8IVFIndex._EXTRA == ()                                           # no list-ordered copy of the codes


def test_the_model_with_every_list_probed_is_the_exhaustive_model():
    """The NumPy model against itself: the index's search over all lists, in any probe order, is gallery_i8_ref.topk of the same
    pair scores - twins in different lists included (the tie goes to the lower row on both sides) - and its slab holds every
    row once."""
    rs = np.random.RandomState(3)
    G, D, Q, nlist = 300, 70, 9, 7
    x = rs.randn(G, D).astype(np.float32)
    x[200] = x[17]                                                                    # twins, in different lists below
    x[5] = 0.0
    x[6, 3] = np.nan
    n = (x / np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True)), 1e-6)).astype(np.float32)
    codes, s_g = R8.quantize_rows(n)
    q = rs.randn(Q, D).astype(np.float32)
    q[0] = x[17]
    qn = (q / np.sqrt((q.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)
    s = R.pair_scores(qn, codes, s_g)
    assign = rs.randint(0, nlist, G)
    assign[17], assign[200] = 5, 1
    offsets, order = I.lists_of(assign, nlist)
    probes = np.stack([rs.permutation(nlist) for _ in range(Q)])
    for k in (1, 3, 150):
        wv, wi = R8.topk(s, k)
        v, i = R.search(s, offsets, order, probes, k)
        assert (i == wi).all() and (v.view(np.int32) == wv.view(np.int32))[~np.isnan(wv)].all() and (np.isnan(v) == np.isnan(wv)).all()
    assert (R8.topk(s, 3)[1][:, 0] == 6).all()                                        # the NaN row first
    top = R8.topk(s[:1], 3)[1][0]
    assert list(top[1:]) == [17, 200]                                                 # the twins, lower row first
    val, idx = R.slab(s, offsets, order, probes, G + 5)
    assert (np.sort(idx[:, :G], axis=1) == np.arange(G)[None, :]).all() and (idx[:, G:] == R.NO_CAND).all()
    assert np.isneginf(val[:, G:]).all()
    v, i = R.search(s, offsets, order, probes[:, :2], 150)                            # two lists: fewer rows, pads behind them
    n_q = np.array([np.isin(assign, p).sum() for p in probes[:, :2]])
    assert ((i >= 0).sum(axis=1) == np.minimum(n_q, 150)).all()
