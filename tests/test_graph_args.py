"""The graph search without a GPU: the ABI names, every limit of mi355_graph_search refused with its message before any HIP
call, its workspace sizer, and the Python argument checks of graph.py."""
import ctypes

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import _lib, graph

NEW = ["mi355_graph_search", "mi355_graph_search_workspace_bytes"]
P = 0x1000        # a non-null, 16-byte aligned address that no check may dereference


def test_new_entries_are_declared_bound_and_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name
    assert _lib.lib().mi355_abi_version() == 3
    assert M.GraphIndex is graph.GraphIndex and M.merged_graph is graph.merged_graph and hasattr(M.Gallery, "graph")
    assert "GraphIndex" not in M.__all__                       # lazy, like PQGallery: the stream table enumerates __all__


def _fails(status, word):
    msg = _lib.lib().mi355_last_error()
    assert status != 0 and word.encode() in msg, (status, msg)


def _search(q=P, Q=3, dim=8, rows=P, dtype=_lib.DTYPE_F32, ld=8, G=100, graph=P, degree=8, seeds=P, nseed=4, k=3, ef=16,
            max_iters=32, filt=None, ov=P, oi=P, it=P, vis=P, ws=P, wsb=1 << 30):
    return _lib.lib().mi355_graph_search(q, Q, dim, 1e-6, rows, dtype, ld, G, graph, degree, seeds, nseed, k, ef, max_iters, 0, filt,
                                         ov, oi, it, vis, ws, wsb, None)


def test_every_limit_is_refused_with_its_message():
    for kw in ("q", "rows", "graph", "seeds", "ov", "oi"):
        _fails(_search(**{kw: None}), "null")
    _fails(_search(Q=-1), "Q=")
    _fails(_search(dtype=2), "dtype")
    _fails(_search(ld=7), "ld=")
    # 1 <= k <= ef <= 512
    _fails(_search(k=0), "k=0")
    _fails(_search(k=17), "k <= ef")
    _fails(_search(ef=513, k=3), "ef=513")
    _fails(_search(ef=0, k=0), "k <= ef")
    # 2 <= degree <= 64
    _fails(_search(degree=1), "degree=1")
    _fails(_search(degree=65), "degree=65")
    # 1 <= nseed <= 64
    _fails(_search(nseed=0), "nseed=0")
    _fails(_search(nseed=65), "nseed=65")
    # 1 <= max_iters, nseed + max_iters * degree <= 16384
    _fails(_search(max_iters=0), "max_iters=0")
    _fails(_search(nseed=1, degree=64, max_iters=256), "visited set")             # 1 + 16384
    _fails(_search(nseed=64, degree=2, max_iters=8161), "visited set")            # 64 + 16322
    _fails(_search(max_iters=(1 << 31) - 1), "visited set")                       # no overflow on the way
    # 1 <= dim <= 4096
    _fails(_search(dim=0), "dim=0")
    _fails(_search(dim=4097, ld=4097), "dim=4097")
    # 1 <= G < 2^31
    _fails(_search(G=0), "G=0")
    _fails(_search(G=1 << 31), "2^31")
    # fp16 rows aligned as mi355_ivf_scan requires
    _fails(_search(dtype=_lib.DTYPE_F16, rows=P + 2, ld=64), "16-byte aligned")
    _fails(_search(dtype=_lib.DTYPE_F16, ld=12), "multiple of 8")
    _fails(_search(ws=None, wsb=0), "workspace")
    _fails(_search(wsb=64), "workspace")
    f = _lib.RankFilter()
    f.label_mode = 7
    _fails(_search(filt=ctypes.byref(f)), "label_mode")
    f.label_mode = _lib.LABEL_SAME
    _fails(_search(filt=ctypes.byref(f)), "needs query_labels")
    # the largest shapes pass every check and stop at the workspace
    _fails(_search(nseed=64, degree=64, max_iters=255, k=512, ef=512, dim=4096, ld=4096, G=(1 << 31) - 1, ws=None, wsb=0),
           "workspace")
    _fails(_search(nseed=64, degree=2, max_iters=8160, ws=None, wsb=0), "workspace")
    # no query: nothing to do, whatever the pointers (but the scalar arguments are still checked); the counters may be null
    assert _search(Q=0, q=None, ov=None, oi=None, it=None, vis=None, ws=None, wsb=0) == 0
    _fails(_search(Q=0, nseed=0), "nseed=0")


def test_workspace_is_zero_for_refused_shapes_and_rises_with_the_queries():
    ws = _lib.lib().mi355_graph_search_workspace_bytes
    ok = dict(Q=3, dim=8, nseed=4, ef=16, degree=8, max_iters=32)
    assert ws(*ok.values()) > 0
    for bad in (dict(Q=0), dict(Q=-1), dict(dim=0), dict(dim=4097), dict(nseed=0), dict(nseed=65), dict(ef=0), dict(ef=513),
                dict(degree=1), dict(degree=65), dict(max_iters=0), dict(max_iters=2048), dict(max_iters=(1 << 31) - 1)):
        assert ws(*{**ok, **bad}.values()) == 0, bad
    last = 0
    for Q in (1, 2, 5, 64, 65, 256, 257, 4096):
        now = ws(Q, 1536, 8, 64, 32, 128)
        assert now > last, (Q, now, last)
        last = now
    assert ws(256, 1536, 8, 64, 32, 128) <= 256 * 1536 * 4 + 1024                 # the normalised queries and a flag word


def _fake_index(rows=500, nentry=9, degree=8, gallery_rows=None, dim=4):
    ix = graph.GraphIndex.__new__(graph.GraphIndex)
    g = M.Gallery.__new__(M.Gallery)
    g.rows, g.dim, g.labels = rows if gallery_rows is None else gallery_rows, dim, None
    ix.gallery, ix.rows, ix.nentry, ix.degree = g, rows, nentry, degree
    return ix


def test_python_argument_checks_come_before_any_launch(monkeypatch):
    monkeypatch.setattr(graph, "lib", lambda: pytest.fail("reached the library"))
    ix = _fake_index()
    q = torch.zeros(3, 4)
    for k in (0, -1, 65, 2.0, True, None):
        with pytest.raises(M.MI355Error, match="k out of range"):
            ix.search(q, k)
    with pytest.raises(M.MI355Error, match="k > ef"):
        ix.search(q, 9, ef=8)
    for ef in (0, 513, 64.0, True):
        with pytest.raises(M.MI355Error, match="ef="):
            ix.search(q, 1, ef=ef)
    for nseed in (0, -1, 10, 1.0, True):                                          # nentry = 9
        with pytest.raises(M.MI355Error, match="nseed"):
            ix.search(q, 3, nseed=nseed)
        with pytest.raises(M.MI355Error, match="nseed"):
            ix.seeds(q, nseed)
    with pytest.raises(M.MI355Error, match="nseed"):
        _fake_index(nentry=100).search(q, 3, nseed=65)
    with pytest.raises(M.MI355Error, match="seeds must be"):
        ix.search(q, 3, seeds=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="nseed"):
        ix.search(q, 3, seeds=torch.zeros((3, 65), dtype=torch.int64))
    for max_iters in (0, -3, 1.5, True):
        with pytest.raises(M.MI355Error, match="max_iters"):
            ix.search(q, 3, max_iters=max_iters)
    with pytest.raises(M.MI355Error, match="visited set"):
        ix.search(q, 3, max_iters=2048)                                           # 8 + 2048 * 8 > 16384
    with pytest.raises(M.MI355Error, match="dim="):
        _fake_index(dim=4100).search(torch.zeros(3, 4100), 3)
    with pytest.raises(M.MI355Error, match="stale"):
        _fake_index(gallery_rows=501).search(q, 3)
    with pytest.raises(M.MI355Error, match="GPU"):                                # host tensors: no CPU path
        ix.search(q, 3, seeds=torch.zeros((3, 2), dtype=torch.int64))
    # the default max_iters: 2 * ef, or what the visited set has room for
    assert ix.default_max_iters(64, 8) == 128 and _fake_index(degree=64).default_max_iters(512, 8) == (16384 - 8) // 64
    with pytest.raises(M.MI355Error, match="Gallery"):
        M.GraphIndex(torch.zeros(4, 4), torch.zeros((4, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 4))
    with pytest.raises(M.MI355Error, match="Gallery"):
        M.GraphIndex.build(torch.zeros(4, 4), 2)
    g = M.Gallery.__new__(M.Gallery)
    g.rows = 100
    for degree in (3, 0, 66, 7, 2.0):
        with pytest.raises(M.MI355Error, match="degree"):
            M.GraphIndex.build(g, 4, degree=degree)
    with pytest.raises(M.MI355Error, match="more than"):
        M.GraphIndex.build(_rows(16), 4, degree=32)                               # knn_graph(16) needs 17 rows
    empty = M.Gallery.__new__(M.Gallery)
    empty.rows = 0
    with pytest.raises(M.MI355Error, match="at least one row"):
        M.GraphIndex(empty, torch.zeros((0, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 4))
    g.device = torch.device("cpu")
    for bad in (torch.zeros((100, 2), dtype=torch.int64), torch.zeros((99, 2), dtype=torch.int32),
                torch.zeros((100, 1), dtype=torch.int32), torch.zeros((100, 65), dtype=torch.int32), torch.zeros(200, dtype=torch.int32)):
        with pytest.raises(M.MI355Error, match="graph must be"):
            M.GraphIndex(g, bad, torch.zeros(2, dtype=torch.int64), torch.zeros(2, 4))


def _rows(n):
    g = M.Gallery.__new__(M.Gallery)
    g.rows = n
    return g


def test_shape_checks_of_search(monkeypatch):
    # pretend the tensors are on the GPU: the shapes must be refused before the library is reached
    from imageretrievalresearch_amd import rank
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)
    monkeypatch.setattr(graph, "lib", lambda: pytest.fail("reached the library"))
    ix = _fake_index()
    g = ix.gallery
    g._buf, g.device, g.dtype, g._prepared, g._prepared_rows, g.eps = torch.zeros(500, 4), torch.device("cpu"), torch.float32, None, 0, 1e-6
    q = torch.zeros(3, 4)
    sd = torch.zeros((3, 2), dtype=torch.int64)
    with pytest.raises(M.MI355Error, match="dims differ"):
        ix.search(torch.zeros(3, 5), 3, seeds=sd)
    with pytest.raises(M.MI355Error, match="seeds must be"):
        ix.search(q, 3, seeds=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="integers"):
        ix.search(q, 3, seeds=torch.zeros(3, 2))
    with pytest.raises(M.MI355Error, match="label_filter"):
        ix.search(q, 3, seeds=sd, label_filter="other")
    with pytest.raises(M.MI355Error, match="labels"):
        ix.search(q, 3, seeds=sd, label_filter="same", query_labels=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="exclude"):
        ix.search(q, 3, seeds=sd, exclude=torch.zeros(2, dtype=torch.int64))
